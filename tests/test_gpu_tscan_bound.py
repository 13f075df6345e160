"""The template scan's three tiers (twoview_tscan_kernel): a tile whose pixels all pass the per-pixel bound
goes straight to the look-ups (option tscan_bound = 1, the default), any other tile is verified label by label (tscan_bound =
0: every tile, the behaviour before the bound), and what fails that is walked by twoview_scan_kernel.  The tiers may differ
in who settles a tile, never in a bit of the maps or in a count."""
import numpy as np
import pytest

import cases
import test_tscan_bound_host as HB
from test_gpu_tscan import CASES
from stereoreconstruction_amd import capi, synthetic

pytestmark = pytest.mark.gpu


def _both(ctx, p, arith, tscan=1):
    """{tscan_bound: [(map, stats) per direction]}"""
    out = {}
    try:
        ctx.set_option("tscan", tscan)
        ctx.set_option("arith", arith)
        for tb in (1, 0):
            ctx.set_option("tscan_bound", tb)
            res = []
            for a, b in ((0, 1), (1, 0)):
                ctx.twoview_wta(a, b, p)
                res.append((ctx.download_depth(a), ctx.stats()))
            out[tb] = res
    finally:
        ctx.set_option("tscan_bound", 1)
        ctx.set_option("tscan", 1)
        ctx.set_option("arith", capi.ARITH_DEFAULT)
    return out


def _same(out, what):
    for d in range(2):
        (m1, s1), (m0, s0) = out[1][d], out[0][d]
        assert s1["used_dense_path"] and s0["used_dense_path"], (what, d)
        assert np.array_equal(m1.view(np.uint64), m0.view(np.uint64)), (what, d)
        for k in ("n_eval", "n_pixels", "n_flagged", "n_certified", "scan_tiles_template", "scan_tiles_walked"):
            assert s1[k] == s0[k], (what, d, k, s1[k], s0[k])
        assert s0["scan_tiles_bound"] == 0, (what, d, s0)
        assert 0 <= s1["scan_tiles_bound"] <= s1["scan_tiles_template"], (what, d, s1)


def _d0_64_case():
    W, H, D, d0 = 200, 36, 24, 64
    L, R, ml, mr, _ = synthetic.rectified_pair(W, H, D, 0x5EED0A64, d0=d0)
    mr = mr.copy(); mr[::2, 0] = 0
    (Kl, Rl, tl), (Kr, Rr, tr) = synthetic.rectified_cameras(W, H)
    zmin, zmax = synthetic.rectified_depth_range(W, D, d0=d0)
    return dict(name="d0_64", kind="twoview", gt_disparity=None,
                views=[(L, ml, (Kl, Rl, tl), None, None), (R, mr, (Kr, Rr, tr), None, None)],
                params=dict(min_depth=zmin, max_depth=zmax, num_depth_levels=D, window_radius=5, weight_kind=1, image_scale=1.0))


@pytest.mark.parametrize("name,over", CASES + [("d0_64", None)])
@pytest.mark.parametrize("arith", [capi.ARITH_CERTIFIED, capi.ARITH_EXACT], ids=["certified", "exact"])
def test_bound_tier_equals_the_label_by_label_tier(hip_ctx, name, over, arith):
    case = _d0_64_case() if name == "d0_64" else cases.get_twoview(name, **over)
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    out = _both(hip_ctx, p, arith)
    _same(out, (name, over))
    for d in range(2):
        assert out[1][d][1]["scan_tiles_bound"] > 0, (name, over, d, out[1][d][1])


def test_a_verged_rig_is_still_walked_and_refuted(hip_ctx):
    """force_dense proposes the dense plan for a verged pair: no pixel passes the bound (nor the label-by-label tier), every
    tile is walked, the walk refutes the plan and the pass is redone on the general kernels -- the map is unchanged."""
    case = cases.get_twoview("adaptive_verged", w=72, h=44, D=20, radius=5)
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    hip_ctx.twoview_wta(0, 1, p)
    want = hip_ctx.download_depth(0)
    hip_ctx.set_option("force_dense", 1)
    try:
        for tb in (1, 0):
            hip_ctx.set_option("tscan_bound", tb)
            hip_ctx.twoview_wta(0, 1, p)
            st = hip_ctx.stats()
            assert not st["used_dense_path"], (tb, st)
            assert np.array_equal(hip_ctx.download_depth(0).view(np.uint64), want.view(np.uint64)), tb
    finally:
        hip_ctx.set_option("tscan_bound", 1)
        hip_ctx.set_option("force_dense", 0)


def test_negative_margin_against_the_oracle(hip_ctx):
    import oracle_ffi as O
    case = cases.get_twoview("geodesic_rect", w=120, h=40, D=40)
    case["params"] = dict(case["params"], wta_margin=-0.5)
    imgs, ocams, op = cases.oracle_inputs(case)
    cams, p = cases.hip_inputs(case)
    assert p.wta_margin == -0.5 and op.wta_margin == -0.5
    cases.upload_case(hip_ctx, case, cams)
    want = O.twoview_wta(imgs[0], imgs[1], ocams[0], ocams[1], op)
    out = _both(hip_ctx, p, capi.ARITH_CERTIFIED)
    _same(out, "negative margin")
    assert out[1][0][1]["scan_tiles_bound"] > 0 and out[1][0][1]["n_certified"] == 0
    ok, msg, _ = cases.compare_depth(out[1][0][0], want, 1e-9)
    assert ok, msg


def _tier2_rig():
    """A rectified 128 x 24 pair, D = 16, whose baseline is chosen -- with the host entry point and the exact replay of the
    reference's chain (test_tscan_bound_host) -- so that the LAST label's x2 at the template pixel lies `room` above an
    integer, with  max eU of a tile's pixels < room < min E of all pixels:  no pixel passes the per-pixel bound (its E does
    not fit the column room), while the label-by-label tier, which needs only eU of room, settles that tile."""
    W, H, D, d0 = 128, 24, 16, 8
    tx, ty = W // 2, H // 2
    (Kl, Rl, tl), _ = synthetic.rectified_cameras(W, H)
    zmin, zmax = synthetic.rectified_depth_range(W, D, d0=d0)
    p = capi.params_twoview(min_depth=zmin, max_depth=zmax, num_depth_levels=D, window_radius=2, weight_kind=1)
    cl = capi.camera_from_krt(Kl, Rl, tl)
    tnums = [HB.label_tnum(cl, p, d) for d in range(D)]

    def right(B):
        (_, _, _), (Kr, Rr, tr) = synthetic.rectified_cameras(W, H, baseline=B)
        return (Kr, Rr, tr), capi.camera_from_krt(Kr, Rr, tr)

    def signed_room(B):
        x2 = HB.project_labels(cl, right(B)[1], p, tnums, tx, ty)[D - 1][0]
        return x2 - round(x2)

    def window(B):
        cr = right(B)[1]
        info = [[capi.tscan_bound(cl, cr, p, (tx, ty), (x, y)) for x in range(W)] for y in range(H)]
        lo = min(max(b["eU"] for b in row[x0:x0 + 64]) for row in info for x0 in (0, 64))
        hi = min(b["E"] for row in info for b in row)
        return lo, hi, info

    # the last label is the farthest plane, disparity d0 B: half a pixel more puts its x2 = x + 0.5 - disparity on an integer
    B0 = 1.0 + 0.5/d0
    lo, hi, _ = window(B0)
    target = 0.5*(lo + hi)
    a, b = B0*(1 - 1e-6), B0*(1 + 1e-6)                 # x2 falls as B grows: signed_room(a) > target > signed_room(b)
    assert signed_room(a) > target > signed_room(b)
    for _ in range(80):
        m = 0.5*(a + b)
        if signed_room(m) > target: a = m
        else: b = m
    return W, H, D, p, cl, right(a), window(a), signed_room(a)


def test_tier_two_is_exercised(hip_ctx):
    """Column room between eU and E (see _tier2_rig): the statistics show tiles settled by the template that the bound did
    NOT settle; the maps equal the curve walk's (tscan = 0) and the oracle's."""
    import oracle_ffi as O
    W, H, D, p, cl, ((Kr, Rr, tr), cr), (lo, hi, info), room = _tier2_rig()
    # the window exists and the baseline found sits in it (host arithmetic; if eU and E ever coincided this would say so)
    assert lo < hi, (lo, hi)
    assert lo < room < hi, (lo, room, hi)
    assert abs(info[0][0]["room_col"] - room) < 1e-13 and not any(b["passes"] for row in info for b in row)
    L, R, ml, mr, _ = synthetic.rectified_pair(W, H, D, 0x5EED0B17)
    (Kl, Rl, tl), _ = synthetic.rectified_cameras(W, H)
    case = dict(name="tier2", kind="twoview", gt_disparity=None,
                views=[(L, ml, (Kl, Rl, tl), None, None), (R, mr, (Kr, Rr, tr), None, None)],
                params=dict(min_depth=p.min_depth, max_depth=p.max_depth, num_depth_levels=D, window_radius=2, weight_kind=1, image_scale=1.0))
    imgs, ocams, op = cases.oracle_inputs(case)
    cams, hp = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    want = O.twoview_wta(imgs[0], imgs[1], ocams[0], ocams[1], op)
    out = _both(hip_ctx, hp, capi.ARITH_CERTIFIED)
    _same(out, "tier 2")
    s1 = out[1][0][1]
    assert s1["scan_tiles_template"] > 0 and s1["scan_tiles_bound"] < s1["scan_tiles_template"], s1
    walk = _both(hip_ctx, hp, capi.ARITH_CERTIFIED, tscan=0)
    for d in range(2):
        assert np.array_equal(out[1][d][0].view(np.uint64), walk[1][d][0].view(np.uint64)), d
        assert out[1][d][1]["n_eval"] == walk[1][d][1]["n_eval"], d
    ok, msg, _ = cases.compare_depth(out[1][0][0], want, 1e-9)
    assert ok, msg


def test_one_size_above_toy(hip_ctx):
    """1920 x 64, D = 256: 30 tiles per row, more tiles than persistent workgroups take in one round"""
    W, H, D = 1920, 64, 256
    L, R, ml, mr, _ = synthetic.rectified_pair(W, H, D, 0x5EED0B03)
    (Kl, Rl, tl), (Kr, Rr, tr) = synthetic.rectified_cameras(W, H)
    zmin, zmax = synthetic.rectified_depth_range(W, D)
    hip_ctx.upload_view(0, L, ml, capi.camera_from_krt(Kl, Rl, tl))
    hip_ctx.upload_view(1, R, mr, capi.camera_from_krt(Kr, Rr, tr))
    p = capi.params_twoview(min_depth=zmin, max_depth=zmax, num_depth_levels=D, weight_kind=capi.WEIGHT_GEODESIC)
    out = _both(hip_ctx, p, capi.ARITH_CERTIFIED)
    _same(out, "1920x64")
    for d in range(2):
        s1 = out[1][d][1]
        assert s1["scan_tiles_template"] == 30*H and s1["scan_tiles_walked"] == 0 and s1["scan_tiles_bound"] > 0, (d, s1)
