"""Tiny and thin views for the parity tests: images narrower or shorter than their own support window, narrower than
one tile of any kernel, with more candidates than columns, and on the tile edges of the dense plan (31/32/33, 63/64/65).

Built like cases.twoview_case / cases.mvs_case, but with the nearest candidate at disparity 1 (d0 = 1): the default
d0 = 8 puts every candidate outside an image narrower than 9 pixels.  Only numpy here."""
import numpy as np

import cases
from stereoreconstruction_amd import synthetic as S

# (w, h, D)
TWOVIEW_SHAPES = [(1, 1, 2), (1, 9, 2), (9, 1, 4), (2, 2, 2), (3, 2, 3), (5, 5, 3), (7, 3, 4), (8, 8, 6), (9, 4, 8),
                  (10, 11, 6), (11, 10, 8), (12, 12, 8), (16, 1, 8), (31, 5, 12), (32, 4, 12), (33, 9, 40), (63, 13, 8),
                  (64, 8, 8), (65, 12, 8), (40, 3, 64)]
# (radius, weight kind): 11 x 11 geodesic windows and 5 x 5 adaptive ones
TWOVIEW_KINDS = [(5, 1), (2, 0)]
MVS_SHAPES = [(3, 3, 4), (5, 4, 6), (8, 8, 8), (9, 7, 8), (12, 9, 8), (16, 5, 8), (31, 9, 12), (33, 7, 12), (65, 6, 8),
              (7, 33, 8)]
# (weight kind, distortion)
MVS_KINDS = [(1, False), (0, True)]
TILE_EDGE_WIDTHS = (31, 32, 33, 63, 64, 65)


def shape_id(s):
    return "x".join(str(v) for v in s)


def small_twoview(w, h, D, radius, weight_kind, masks=False, verged=False, distortion=False):
    L, R, ml, mr, disp = S.rectified_pair(w, h, D, 0x5EED0E00 + 131 * w + h, d0=1)
    (Kl, Rl, tl), (Kr, Rr, tr) = S.rectified_cameras(w, h)
    zmin, zmax = S.rectified_depth_range(w, D, d0=1)
    if verged:
        # the perturbations of cases.twoview_case: its numbers COPIED (that builder takes no d0), not shared -- a change there
        # does not reach this file
        Rr = cases._rot_z(0.05) @ cases._rot_x(0.02) @ cases._rot_y(-0.04)
        tr = -Rr @ np.array([1.0, 0.03, 0.02])
        Rl = cases._rot_y(0.03)
        tl = -Rl @ np.zeros(3)
    dist_l = dist_r = None
    if distortion:
        # (copied from cases.twoview_case as well)
        dist_l = np.array([-0.131, 0.4, 0.004, 0.003, -0.6])
        dist_r = np.array([-0.058, -0.2, 0.0, 0.006, 0.3])
    if masks:
        yy, xx = np.mgrid[0:h, 0:w]
        ml = ((xx + 2 * yy) % 5 != 0).astype(np.uint8)
        mr = ((2 * xx + yy) % 7 != 0).astype(np.uint8)
    params = dict(min_depth=zmin, max_depth=zmax, num_depth_levels=D, window_radius=radius, weight_kind=weight_kind,
                  image_scale=1.0)
    views = [(L, ml, (Kl, Rl, tl), dist_l, None), (R, mr, (Kr, Rr, tr), dist_r, None)]
    name = "small_%dx%dx%d_r%d_k%d%s%s%s" % (w, h, D, radius, weight_kind, "_masks" if masks else "",
                                             "_verged" if verged else "", "_dist" if distortion else "")
    return dict(name=name, kind="twoview", views=views, params=params, gt_disparity=disp)


def small_mvs(w, h, D, weight_kind, distortion):
    return cases.mvs_case("small_mvs_%dx%dx%d_k%d%s" % (w, h, D, weight_kind, "_dist" if distortion else ""),
                          nviews=3, w=w, h=h, D=D, weight_kind=weight_kind, radius=2, distortion=distortion)


# the shape groups every path of the library has to have run in (tests/test_gpu_small_shapes.py)
def groups(shape, radius):
    w, h, D = shape
    g = []
    if w <= 2 * radius:
        g.append("w<=2r")
    if h <= 2 * radius:
        g.append("h<=2r")
    if D > w:
        g.append("D>w")
    if w in TILE_EDGE_WIDTHS:
        g.append("tile edge")
    return g
