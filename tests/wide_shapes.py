"""Wide and tall views for the parity tests: the other end of tests/small_shapes.py.  Widths and heights on either side of
the powers of two at which a 16-bit field, a grid size or a 32-bit index could change (2048, 4096, 8192, 16384) up to
M = capi.MAX_VIEW_DIM, the largest side srh_view_upload accepts, a few rows or columns thick so that the
CPU oracle of one direction stays within a few seconds.

Built on small_shapes.small_twoview (its d0 = 1, its seeds).  The general rig is this file's own: see general_cameras."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import cases
import small_shapes as SS
from stereoreconstruction_amd import capi
from stereoreconstruction_amd import synthetic as S

M = capi.MAX_VIEW_DIM

# (w, h, D).  The heights of the wide shapes (and the widths of the tall ones) are what keeps one oracle direction at
# r = 5 geodesic within about 5 s on one thread per row; none had to be lowered from the values first chosen.
WIDE_SHAPES = [(2049, 5, 8), (4097, 6, 8), (8200, 4, 8), (16400, 3, 8), (M, 2, 8), (M, 3, 12)]
TALL_SHAPES = [(5, 2049, 4), (4, 8200, 4), (3, 16400, 3), (2, M, 2), (3, M, 3)]
# a long candidate range on a wide view: the dense plan's cstride (304) + one tile is beyond the strip kernel's chunk of
# 320 columns, so the per-tile kernel runs by the host's choice
LONG_RANGE_SHAPE = (8200, 3, 300)
TWOVIEW_SHAPES = WIDE_SHAPES + TALL_SHAPES + [LONG_RANGE_SHAPE]
# general geometry runs at every wide and tall shape
GENERAL_SHAPES = WIDE_SHAPES + TALL_SHAPES
TWOVIEW_KINDS = SS.TWOVIEW_KINDS
# MultiViewStereo: (w, h, D), three views.  The oracle's estimate grows with w^2: the first two are compared with it, the
# M shapes compare the device's kernels with each other
MVS_ORACLE_SHAPES = [(2049, 5, 8), (5, 2049, 8)]
MVS_DEVICE_SHAPES = [(M, 5, 8), (5, M, 8)]

shape_id = SS.shape_id


def is_wide(shape):
    return shape[0] >= shape[1]


def general_cameras(w, h):
    """A verged pinhole rig after small_twoview's, its angles sized in PIXELS moved, so that a view a few rows (or
    columns) thick keeps its candidates.  small_twoview's own numbers turn a 32767-wide row by 1600 rows at its ends: 291
    of 98400 pixels keep a candidate at 32800x3.

    F = max(w, h) is the focal length (for a wide view small_twoview's own f = w; a tall view with f = w = 3 would be a
    camera with rays 5000 focal lengths off its axis), n = min(w, h) the thin side.
      wide: rot_z and rot_x and the baseline's y are small_twoview's scaled by 64 / F -- a row's ends move by +- 1.6 rows
            and the whole row by 1.28 as at width 64 -- but by no more than n / 8 rows each, so that a two-row view keeps
            more than half its candidates; rot_y (along the rows) keeps small_twoview's angles;
      tall: the columns are the scarce side: rot_z moves a column's ends by +- n / 16 columns, the left rot_y by n / 24
            columns, the right one verges by 3/4 of a column -- it takes most of the nearest candidate's disparity of 1
            back, without which a two-column view has no candidate right to left in its last column; rot_x moves every
            row by 1.28 rows.  A curve then crosses a handful of rows: the row-run lists (at most 32 rows per curve) stand.
    No distortion: its radial terms grow with the cube of the half-width over the focal length, not with an angle."""
    F, n = float(max(w, h)), float(min(w, h))
    K = np.array([[F, 0, w / 2.0], [0, F, h / 2.0], [0, 0, 1.0]])
    if w >= h:
        az, ax = min(3.2, n / 4.0) / F, min(1.28, n / 8.0) / F
        ayr, ayl = -0.04, 0.03
    else:
        az, ax = (n / 8.0) / F, 1.28 / F
        ayr, ayl = 0.75 / F, (n / 24.0) / F
    Rr = cases._rot_z(az) @ cases._rot_x(ax) @ cases._rot_y(ayr)
    tr = -Rr @ np.array([1.0, 0.03 * 64.0 / F, 0.02])
    Rl = cases._rot_y(ayl)
    tl = -Rl @ np.zeros(3)
    return (K, Rl, tl), (K.copy(), Rr, tr)


def band_mask(w, h):
    """WHITE in 160 columns at either end of the rows and 160 either side of every power of two from 2048 up: the columns
    at which a field or a tile count could change, a fifth of a view 8200 wide"""
    keep = np.zeros(w, bool)
    keep[:160] = keep[-160:] = True
    p2 = 2048
    while p2 < w:
        keep[p2 - 160:p2 + 160] = True
        p2 *= 2
    return np.repeat(keep[None, :], h, 0).astype(np.uint8)


def wide_twoview(w, h, D, radius, weight_kind, masks=False, general=False):
    """small_twoview at a wide or tall shape.  masks: its two modulo patterns -- at LONG_RANGE_SHAPE band_mask on both
    views instead: the oracle takes 12 s for ONE row of 8200 pixels x 300 candidates at r = 5, whatever the height, so
    that shape is compared with the oracle on a fifth of its columns (and with the walk kernel on all of them)."""
    case = SS.small_twoview(w, h, D, radius, weight_kind, masks=masks)
    if masks and (w, h, D) == LONG_RANGE_SHAPE:
        case["views"] = [(v[0], band_mask(w, h)) + tuple(v[2:]) for v in case["views"]]
    if general:
        cams = general_cameras(w, h)
        case["views"] = [(v[0], v[1], cam, None, None) for v, cam in zip(case["views"], cams)]
        # the depths of disparities 1 .. D under the rig's focal length
        zmin, zmax = S.rectified_depth_range(max(w, h), D, d0=1)
        case["params"].update(min_depth=zmin, max_depth=zmax)
    case["name"] = "wide" + case["name"][len("small"):] + ("_general" if general else "")
    return case


def wide_mvs(w, h, D, weight_kind, nviews=3):
    """cases.mvs_case's scene (three cameras on a semicircle around the textured sphere, its depth range and threshold) with
    the focal length taken from the LONG side -- under mvs_case's 1.4 w the sphere of a view 5 columns wide is 9 pixels --
    and, for a tall view, every camera rolled a quarter turn about its axis: the epipolar curves then run along the
    columns, the long way through the image, as they run along the rows of a wide one."""
    focal = 1.4 * max(w, h)
    rig = S.semicircle_rig(nviews, w, h, radius=10.0, step_deg=12.0, focal=focal)
    if h > w:
        Q = cases._rot_z(np.pi / 2)
        rig = [(K, Q @ R, Q @ t) for K, R, t in rig]
    views = []
    for v in range(nviews):
        rgba, masks, _ = S.render_sphere_views([rig[v]], w, h, 0x5EED0B00, sphere_radius=2.0, tex_size=256)
        views.append((rgba[0], masks[0], rig[v], None, None))
    zmin, zmax = 7.5, 10.5
    params = dict(min_depth=zmin, max_depth=zmax, num_depth_levels=D, window_radius=2, weight_kind=weight_kind,
                  image_scale=1.0, cross_check_threshold=2.0 * (zmax - zmin) / (D - 1))
    return dict(name="wide_mvs_%dx%dx%d_k%d" % (w, h, D, weight_kind), kind="mvs", views=views, params=params)


def row_bands(h, n=16):
    """[y0, y1) bands of a view's rows, at most n of them"""
    n = min(n, h)
    edges = [(h * k) // n for k in range(n + 1)]
    return [(a, b) for a, b in zip(edges[:-1], edges[1:]) if b > a]


def oracle_wta(O, imgs, ocams, op, ref, oth):
    """the CPU oracle's pass ref -> oth, its rows in bands on up to 16 threads (the C oracle runs outside the GIL):
    (depth, diag) as oracle_ffi.twoview_wta(..., want_diag=True) returns them for the whole view"""
    h = imgs[ref].h
    bands = row_bands(h)
    with ThreadPoolExecutor(max_workers=len(bands)) as ex:
        parts = list(ex.map(lambda b: O.twoview_wta(imgs[ref], imgs[oth], ocams[ref], ocams[oth], op, b[0], b[1], want_diag=True), bands))
    depth, diag = parts[0]
    n_eval = diag["n_eval"]
    for (a, b), (d, g) in list(zip(bands, parts))[1:]:
        depth[a:b] = d[a:b]
        for k in ("win_xy", "min_cost", "second_cost"):
            diag[k][a:b] = g[k][a:b]
        n_eval += g["n_eval"]
    diag["n_eval"] = n_eval
    return depth, diag


def oracle_mvs(O, imgs, ocams, view, neigh, op):
    """the oracle's initial estimate of one view, its rows in bands on up to 16 threads: (depth, n_eval)"""
    bands = row_bands(imgs[view].h)
    with ThreadPoolExecutor(max_workers=len(bands)) as ex:
        parts = list(ex.map(lambda b: O.mvs_initial_estimate(imgs, ocams, view, neigh, op, b[0], b[1]), bands))
    depth, n_eval = parts[0]
    for (a, b), (d, ne) in list(zip(bands, parts))[1:]:
        depth[a:b] = d[a:b]
        n_eval += ne
    return depth, n_eval


def sample_columns(w, half):
    """`half` columns at either end of a row and either side of every power of two from 2048 up"""
    cols = set(range(min(half, w))) | set(range(max(0, w - half), w))
    p2 = 2048
    while p2 < w:
        cols |= set(range(p2 - half, min(w, p2 + half)))
        p2 *= 2
    return sorted(cols)
