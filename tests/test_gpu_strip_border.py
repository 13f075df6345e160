"""The strip kernel's border instantiation (srh_strip.hip, BORDER): the rows whose window the image's top or bottom edge
cuts run the exact two sweeps over the window rows inside the image instead of the blocked select form.

Every case is compared bit for bit with the per-tile kernel (srh_dense.hip, whose select form settles those rows as
before) in the reference's arithmetic, under the certified default and under the reference's arithmetic, in both strip
forms; the default path is also compared with the oracle.  Flat border rows give clipped windows with sum2 = 0 next to
textured ones, masks give pixels and candidates with unusable taps inside the clipped window (they stay in phase 2), a
13-row image has no interior rows at all, and bands that cut the border rows apart exercise the row split of the launch.
"""
import numpy as np
import pytest

import cases
import oracle_ffi as O
from stereoreconstruction_amd import capi

pytestmark = pytest.mark.gpu

RTOL = 1e-9


def _flat_border(case, rows):
    """The top and bottom `rows` rows of both images one gray value: flat clipped windows."""
    views = []
    for (img, mask, cams, dist, plane) in case["views"]:
        img = img.copy()
        img[:rows] = img[rows, 0]
        img[-rows:] = img[-rows - 1, 0]
        views.append((img, mask, cams, dist, plane))
    return dict(case, views=views)


BORDER_CASES = [
    ("geodesic_rect", dict(w=96, h=40, D=40), 0),
    ("adaptive_rect", dict(w=97, h=37, D=24), 0),
    ("geodesic_r2", dict(), 0),
    ("adaptive_rect", dict(w=64, h=30, D=16, radius=2), 0),
    ("geodesic_masks", dict(w=80, h=36, D=20), 0),
    ("geodesic_rect", dict(w=96, h=40, D=40), 7),          # flat border rows: sum2 = 0 next to textured windows
    ("adaptive_rect", dict(w=70, h=24, D=20), 4),
    ("geodesic_rect", dict(w=161, h=13, D=130), 0),        # every row a border row: no main launch; 8-wave form
]


def _run(ctx, p, strip, arith):
    ctx.set_option("strip", strip)
    ctx.set_option("arith", arith)
    out = []
    try:
        for a, b in ((0, 1), (1, 0)):
            ctx.twoview_wta(a, b, p)
            out.append((ctx.download_depth(a), ctx.stats()))
    finally:
        ctx.set_option("strip", 1)
        ctx.set_option("arith", capi.ARITH_DEFAULT)
    return out


@pytest.mark.parametrize("name,over,flat", BORDER_CASES)
def test_border_rows_match_the_per_tile_kernel_and_the_oracle(hip_ctx, name, over, flat):
    case = cases.get_twoview(name, **over)
    if flat:
        case = _flat_border(case, flat)
    imgs, ocams, op = cases.oracle_inputs(case)
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    ref = _run(hip_ctx, p, 0, 0)
    assert not ref[0][1]["used_strip_kernel"] and ref[0][1]["used_dense_path"]
    for strip in (4, 8):
        for arith in (0, capi.ARITH_DEFAULT):
            got = _run(hip_ctx, p, strip, arith)
            for d in range(2):
                assert got[d][1]["used_strip_kernel"], "strip=%d: the strip kernel did not run" % strip
                assert np.array_equal(got[d][0].view(np.uint64), ref[d][0].view(np.uint64)), \
                    "strip=%d arith=%d direction %d: depth bits differ from the per-tile kernel" % (strip, arith, d)
                assert got[d][1]["n_eval"] == ref[d][1]["n_eval"]
    want = O.twoview_wta(imgs[0], imgs[1], ocams[0], ocams[1], op)
    ok, msg, _ = cases.compare_depth(_run(hip_ctx, p, 8, capi.ARITH_DEFAULT)[0][0], want, RTOL)
    assert ok, msg


@pytest.mark.parametrize("strip", [4, 8])
def test_bands_that_start_and_end_inside_the_border_rows(hip_ctx, strip):
    """Row bands that cut the top and bottom border rows apart give the same map as one band."""
    case = cases.get_twoview("geodesic_rect", w=96, h=40, D=24)
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    full = _run(hip_ctx, p, 0, 0)[0][0]
    hip_ctx.set_option("strip", strip)
    try:
        hip_ctx.upload_depth(0, np.full(full.shape, np.nan))
        for y0, y1 in ((0, 3), (3, 8), (8, 36), (36, 38), (38, 40)):
            hip_ctx.twoview_wta(0, 1, p, y0, y1)
            assert hip_ctx.stats()["used_strip_kernel"]
        got = hip_ctx.download_depth(0)
    finally:
        hip_ctx.set_option("strip", 1)
    assert np.array_equal(got.view(np.uint64), full.view(np.uint64))
