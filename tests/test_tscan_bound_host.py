"""The template scan's per-pixel bound (srh_walk.hpp: ts_pixel_setup, ts_pixel_E, ts_pixel_passes) as host
arithmetic, through srh_tscan_bound -- no GPU.

The reference's projection chain of a label (Camera::unproject, pointFromDepth / intersect, Camera::project: the operations
of cam_unproject, pinhole_label_tnum and pinhole_project_label, in their order) is replayed here in `fractions.Fraction`,
every operation formed as a rational and rounded ONCE to a double -- the arithmetic of the reference's x86-64 build, which
never fuses a multiply-add.  Against it, for a few dozen pixels of four canonical rigs and of every rig of tests/rig_cases.py
that the dense plan is proposed for (rotated, displaced, far from the origin, scaled, slots exchanged, one K per view), and
ALL labels:
 (a) |x2(x, y, d) - x2(x_T, y_T, d) - (x - x_T)| <= E, as rationals;
 (b) a pixel the bound passes has the template pixel's states (not projectable / first / dropped / kept) and columns, label
     by label, and every kept point on its own row;
 (c) E is finite and below 2^-20 on the rigs whose every pixel the template serves (rig_cases.RIGS: template "all").
The proof assumes nothing about the rig (no equal intrinsics, no shared camera centre): what it needs it tests per pixel and
answers +inf otherwise, so there is no property of the rig to assert here -- the table's rigs are where that is held:
`half_pixel` (cx_b = cx_a - 0.5: the template's labels land on integer columns, room_col = 0) lets no pixel pass, and
`fx_ratio` (fx_b = 1.07 fx_a: the template is no shift) only pixels of the template's own column."""
import math
from fractions import Fraction as F

import numpy as np
import pytest

import cases
import rig_cases
from stereoreconstruction_amd import capi, synthetic


def fl(fr):
    return float(fr)                                   # Fraction -> float is correctly rounded: one rounding


def add(a, b): return fl(F(a) + F(b))
def sub(a, b): return fl(F(a) - F(b))
def mul(a, b): return fl(F(a) * F(b))
def div(a, b): return fl(F(a) / F(b))


def dsqrt(a):
    return math.sqrt(a)                                # IEEE: correctly rounded


def dot(a, b): return add(add(mul(a[0], b[0]), mul(a[1], b[1])), mul(a[2], b[2]))     # (left to right, srh_geom.hpp)
def matvec(M, v): return [dot(M[0:3], v), dot(M[3:6], v), dot(M[6:9], v)]
def normalized(a):
    n = dsqrt(dot(a, a))
    return [div(a[0], n), div(a[1], n), div(a[2], n)]


def unproject(cam, px, py):
    d = normalized(matvec(list(cam.Kinv), [px, py, 1.0]))
    return matvec(list(cam.Rinv), [sub(0.0, cam.t[0]), sub(0.0, cam.t[1]), sub(0.0, cam.t[2])]), normalized(matvec(list(cam.Rinv), d))


def label_tnum(cam, p, d):
    normal = list(cam.pdir)
    n = normalized(normal)
    t = div(float(d), sub(float(p.num_depth_levels), 1.0))
    t = div(t, sub(5.0, mul(4.0, t)))
    depth = add(mul(p.min_depth, sub(1.0, t)), mul(p.max_depth, t))
    x0 = [add(cam.C[i], mul(normal[i], depth)) for i in range(3)]
    dist = dot(n, x0)
    x0p = [mul(dist, n[i]) for i in range(3)]
    src = matvec(list(cam.Rinv), [sub(0.0, cam.t[0]), sub(0.0, cam.t[1]), sub(0.0, cam.t[2])])
    return dot(n, [sub(x0p[i], src[i]) for i in range(3)])


def project_labels(ref, oth, p, tnums, x, y):
    """[(x2, y2) or None per label]: the reference's chain for pixel (x, y)"""
    sc = p.image_scale
    src, dr = unproject(ref, div(x + 0.5, sc), div(y + 0.5, sc))
    nd = dot(normalized(list(ref.pdir)), dr)
    out = []
    for tn in tnums:
        if abs(nd) < 1e-10:
            out.append(None); continue
        t = div(tn, nd)
        if t < 1e-10:
            out.append(None); continue
        point = [add(src[i], mul(t, dr[i])) for i in range(3)]
        pl = [add(a, b) for a, b in zip(matvec(list(oth.R), point), list(oth.t))]
        pk = matvec(list(oth.K), pl)
        out.append((mul(div(pk[0], pk[2]), sc), mul(div(pk[1], pk[2]), sc)))
    return out


def keep_chain(pts):
    """TwoViewStereo::epipolarCurve's decisions per label: (state, column, row); state 0 not projectable, 1 first point,
    2 dropped by the one-pixel test, 3 kept; column / row truncated towards zero as the reference's int conversion does"""
    res, last = [], None
    for q in pts:
        if q is None:
            res.append((0, None, None)); continue
        if last is None:
            last = q; res.append((1, int(q[0]), int(q[1]))); continue
        dx, dy = sub(q[0], last[0]), sub(q[1], last[1])
        if not (add(mul(dx, dx), mul(dy, dy)) >= 1):
            res.append((2, None, None)); continue
        last = q; res.append((3, int(q[0]), int(q[1])))
    return res


def _rig(name):
    if name == "c3":
        W, H, D = 1920, 1080, 256
        cams = [capi.camera_from_krt(*c) for c in synthetic.rectified_cameras(W, H)]
        zmin, zmax = synthetic.rectified_depth_range(W, D)
        return W, H, cams, capi.params_twoview(min_depth=zmin, max_depth=zmax, num_depth_levels=D, weight_kind=capi.WEIGHT_GEODESIC)
    if name == "d0_64":
        W, H, D, d0 = 200, 36, 24, 64
        cams = [capi.camera_from_krt(*c) for c in synthetic.rectified_cameras(W, H)]
        zmin, zmax = synthetic.rectified_depth_range(W, D, d0=d0)
        return W, H, cams, capi.params_twoview(min_depth=zmin, max_depth=zmax, num_depth_levels=D, window_radius=5, weight_kind=1)
    if name.startswith("rig_"):
        case = rig_cases.rig_twoview(name[4:])
        cams, p = cases.hip_inputs(case)
        h, w = case["views"][0][1].shape
        return w, h, cams, p
    case = cases.get_twoview({"scaled": "geodesic_scaled", "masks": "geodesic_masks"}[name])
    cams, p = cases.hip_inputs(case)
    h, w = case["views"][0][1].shape
    return w, h, cams, p


def _pixels(W, H, tx, ty, seed, n_random):
    rng = np.random.default_rng(seed)
    px = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (tx, ty), (tx + 1, ty), (0, ty), (W - 1, ty), (0, H // 3), (W - 1, 2 * H // 3),
          (W // 3, 0), (2 * W // 3, H - 1)]
    px += [(x, H // 4) for x in (63, 64) if x < W]                    # either side of the 64-pixel scan tile's edge
    px += [(int(rng.integers(0, W)), int(rng.integers(0, H))) for _ in range(n_random)]
    return px


def _template(rig):
    """which pixels the bound lets pass on this rig: the canonical rigs serve all of theirs"""
    return rig_cases.RIGS[rig[4:]]["template"] if rig.startswith("rig_") else "all"


@pytest.mark.parametrize("rig,n_random", [("c3", 12), ("d0_64", 28), ("scaled", 28), ("masks", 28)] + [("rig_" + n, 28) for n in rig_cases.PROPOSED])
@pytest.mark.parametrize("direction", [0, 1])
def test_bound_holds_for_every_label(rig, n_random, direction):
    W, H, cams, p = _rig(rig)
    ref, oth = cams[direction], cams[1 - direction]
    D = p.num_depth_levels
    tnums = [label_tnum(ref, p, d) for d in range(D)]
    tx, ty = W // 2, H // 2                            # twoview_template_kernel's pixel for a band of all rows
    tpts = project_labels(ref, oth, p, tnums, tx, ty)
    tchain = keep_chain(tpts)
    n_pass = 0
    for (x, y) in _pixels(W, H, tx, ty, 0x7E5CA0 + direction, n_random):
        b = capi.tscan_bound(ref, oth, p, (tx, ty), (x, y))
        E = b["E"]
        if _template(rig) == "all":
            assert math.isfinite(E) and E < 2.0 ** -20, (rig, x, y, b)                  # (c)
        if _template(rig) == "none":
            assert b["room_col"] == 0 and not b["passes"], (rig, x, y, b)
        if _template(rig) == "column":
            assert not b["passes"] or x == tx, (rig, x, y, b)
        assert b["eU"] <= E and b["eU_template"] <= E
        pts = project_labels(ref, oth, p, tnums, x, y)
        for d in range(D):                                                             # (a)
            assert (pts[d] is None) == (tpts[d] is None), (rig, x, y, d)
            if pts[d] is not None:
                assert abs(F(pts[d][0]) - F(tpts[d][0]) - (x - tx)) <= F(E), (rig, x, y, d, pts[d], tpts[d], E)
        if b["passes"]:                                                                # (b)
            n_pass += 1
            chain = keep_chain(pts)
            for d in range(D):
                st, col, row = chain[d]
                tst, tcol, _ = tchain[d]
                assert st == tst, (rig, x, y, d, st, tst)
                if st in (1, 3):
                    # the template's FLOOR column shifted by x - x_T; the reference's truncation towards zero is one to the
                    # right of the floor left of the image
                    want = math.floor(tpts[d][0]) + (x - tx)
                    assert col == want + (1 if pts[d][0] < 0 else 0), (rig, x, y, d, col, want)
                    assert row == y, (rig, x, y, d, row)
    assert n_pass > 0 or _template(rig) == "none", rig  # (the verdict is exercised; on `fx_ratio` by the template pixel itself)


def test_rooms_are_the_template_pixels_own():
    """the three rooms against the exact replay of the template pixel's chain"""
    W, H, cams, p = _rig("d0_64")
    D = p.num_depth_levels
    tnums = [label_tnum(cams[0], p, d) for d in range(D)]
    tx, ty = W // 2, H // 2
    pts = project_labels(cams[0], cams[1], p, tnums, tx, ty)
    chain = keep_chain(pts)
    col, one, last = F(1, 2), None, None
    for q, (st, _, _) in zip(pts, chain):
        if st in (1, 3):
            fr = F(q[0]) - math.floor(q[0])
            col = min(col, fr, 1 - fr)
        if st in (2, 3):
            adx = abs(F(sub(q[0], last[0])))
            room = F(0) if (st == 3 and adx < 1) else abs(adx - 1)
            one = room if one is None else min(one, room)
        if st in (1, 3):
            last = q
    b = capi.tscan_bound(cams[0], cams[1], p, (tx, ty), (3, 5))
    assert b["template_ok"] == 1 and b["pixel_ok"] == 1
    assert abs(F(b["room_col"]) - col) <= F(2) ** -52 and abs(F(b["room_one"]) - one) <= F(2) ** -52, (b, float(col), float(one))
    nd = dot(normalized(list(cams[0].pdir)), unproject(cams[0], tx + 0.5, ty + 0.5)[1])
    assert b["room_proj"] == sub(min(div(tn, nd) for tn in tnums), 1e-10)


def test_a_verged_rig_does_not_pass():
    case = cases.get_twoview("adaptive_verged", w=72, h=44, D=20, radius=5)
    cams, p = cases.hip_inputs(case)
    for xy in ((0, 0), (36, 22), (37, 22), (71, 43)):
        b = capi.tscan_bound(cams[0], cams[1], p, (36, 22), xy)
        assert b["passes"] == 0, (xy, b)
