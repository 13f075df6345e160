"""Depth-map fusion on the device (srh_mvs_fuse, srh_fuse.hip) against its CPU restatement (tests/fuse_ref.py), whose
geometry is the oracle's: counters, sources, view counts, flags and colours exactly, positions bit for bit, normals
within 1e-12.  The inputs are analytic depth maps (every pixel's oracle ray cut with the scene's sphere) with every kind
of hole; tests/test_fuse_host.py checks, without a GPU, that they exercise every branch and sit on no threshold."""
import ctypes as C

import numpy as np
import pytest

import cases
import fuse_ref as F
import oracle_ffi as O
from stereoreconstruction_amd import capi

pytestmark = pytest.mark.gpu

COUNTERS = ("n_points", "n_candidates", "n_claimed", "n_unsupported", "n_normals")
ARRAYS = ("xyz", "normals", "rgb", "nviews", "flags", "src")


def _upload(ctx, I, order=None, depths=None):
    """The case's views into slots 0.. (in `order`), with their depth maps -> srh_params."""
    case = I["case"]
    cams, p = cases.hip_inputs(case)
    n = len(cams)
    order = list(range(n)) if order is None else list(order)
    depths = I["depths"] if depths is None else depths
    for slot, v in enumerate(order):
        rgba, mask = case["views"][v][:2]
        ctx.upload_view(slot, rgba, mask, cams[v])
        ctx.upload_depth(slot, depths[v])
    return p


_assert_equal = F.assert_equal


def _npix(I, order=None):
    n = [m.size for m in I["masks"]]
    return n if order is None else [n[v] for v in order]


@pytest.mark.parametrize("name,over", [pytest.param(name, {}, id=name) for name in F.FUSE_CASES]
                         + [pytest.param(name, over, id="%s-%dx%dx%d" % (name, over["nviews"], over["w"], over["h"]))
                            for name, over in F.FUSE_SIZE_CASES])
def test_fusion_equals_the_restatement(hip_ctx, name, over):
    I = F.case_inputs(name, **over)
    want = F.case_result(name, **over)
    p = _upload(hip_ctx, I)
    n = len(I["ocams"])
    got = hip_ctx.mvs_fuse(list(range(n)), p, capi.fuse_params(dist_threshold=I["thr"]))
    _assert_equal(got, want, name, _npix(I))
    assert got["n_candidates"] == got["n_points"] + got["n_claimed"] + got["n_unsupported"]
    assert hip_ctx.mvs_fused_count() == want["n_points"]


def test_list_order_and_slots(hip_ctx):
    """The slot list's order is the order of the rule, and `src` counts list entries, not slots."""
    name = "mvs_geodesic"
    I = F.case_inputs(name)
    n = len(I["ocams"])
    rev = list(reversed(range(n)))
    p = _upload(hip_ctx, I)
    got = hip_ctx.mvs_fuse(rev, p, capi.fuse_params(dist_threshold=I["thr"]))
    _assert_equal(got, F.case_result(name, order=rev), "reversed")


@pytest.mark.parametrize("min_views", [3, 4])
def test_more_than_two_views_required(hip_ctx, min_views):
    name = "mvs_geodesic"
    I = F.case_inputs(name)
    n = len(I["ocams"])
    assert n == 4
    want = F.case_result(name, min_views=min_views)
    p = _upload(hip_ctx, I)
    got = hip_ctx.mvs_fuse(list(range(n)), p, capi.fuse_params(dist_threshold=I["thr"], min_views=min_views))
    _assert_equal(got, want, "min_views %d" % min_views, _npix(I))
    assert got["n_points"] > 0 and got["nviews"].min() >= min_views and got["nviews"].max() == n


@pytest.mark.parametrize("fraction", F.GAP_FRACTIONS)
def test_explicit_normal_depth_gap(hip_ctx, fraction):
    """srh_fuse_params.normal_depth_gap below the default: fewer neighbours are usable, fewer points have a tangent."""
    name = "mvs_geodesic"
    I = F.case_inputs(name)
    n = len(I["ocams"])
    gap = F.default_gap(I["op"]) / fraction
    want = F.case_result(name, gap=gap)
    p = _upload(hip_ctx, I)
    got = hip_ctx.mvs_fuse(list(range(n)), p, capi.fuse_params(dist_threshold=I["thr"], normal_depth_gap=gap))
    _assert_equal(got, want, "gap 1/%d of the default" % fraction, _npix(I))
    assert 0 < got["n_normals"] < F.case_result(name)["n_normals"]


@pytest.mark.parametrize("over,order", F.MIXED_ORDERS, ids=[
    "%s-%d%d%d" % (("%dx%d" % (o["w"], o["h"]) if o else "default",) + tuple(q)) for o, q in F.MIXED_ORDERS])
def test_largest_view_not_first(hip_ctx, over, order):
    """Lists whose first entry is not the largest view: the scratch is sized by the largest (pixels and blocks), and a short
    view's scan runs over a block_counts array that still holds a longer view's counts behind its own."""
    name = "mvs_mixed_sizes"
    I = F.case_inputs(name, **over)
    want = F.case_result(name, order=order, **over)
    p = _upload(hip_ctx, I)                                            # view v in slot v; the list gives the order
    got = hip_ctx.mvs_fuse(list(order), p, capi.fuse_params(dist_threshold=I["thr"]))
    _assert_equal(got, want, "order %s" % (order,), _npix(I, order))


def test_single_view_is_the_views_own_cloud(hip_ctx):
    I = F.case_inputs("mvs_distorted")
    p = _upload(hip_ctx, I)
    pc = hip_ctx.point_cloud(1, p)
    got = hip_ctx.mvs_fuse([1], p, capi.fuse_params(min_views=1))
    valid = pc["valid"].ravel() == 1
    assert got["n_points"] == pc["n_points"] == int(valid.sum()) > 0
    assert got["n_claimed"] == 0 and got["n_unsupported"] == 0
    assert np.array_equal(got["src"][:, 0], np.zeros(got["n_points"], np.int32))
    assert np.array_equal(got["src"][:, 1], np.flatnonzero(valid).astype(np.int32))
    assert np.array_equal(got["xyz"].view(np.uint64), pc["xyz"].reshape(-1, 3)[valid].view(np.uint64))
    assert np.array_equal(got["rgb"], pc["rgb"].reshape(-1, 3)[valid])
    assert np.all(got["nviews"] == 1)
    nrm = got["normals"]
    assert np.abs(np.sqrt((nrm * nrm).sum(1)) - 1.0).max() <= 1e-12
    Cc = np.array(I["ocams"][1].C[:])
    assert np.all((nrm * (Cc[None, :] - got["xyz"])).sum(1) >= 0)
    # with the default min_views = 2 a lone view supports nothing
    alone = hip_ctx.mvs_fuse([1], p)
    assert alone["n_points"] == 0 and alone["n_unsupported"] == alone["n_candidates"] == pc["n_points"]


def test_holes_and_empty_results(hip_ctx):
    name = "mvs_refractive"
    I = F.case_inputs(name)
    n = len(I["ocams"])
    depths = [d.copy() for d in I["depths"]]
    depths[1][:] = np.nan                                              # one view without a single point
    p = _upload(hip_ctx, I, depths=depths)
    f = capi.fuse_params(dist_threshold=I["thr"])
    got = hip_ctx.mvs_fuse(list(range(n)), p, f)
    want = F.fuse(I["ocams"], I["op"], I["rgbas"], I["masks"], depths, I["thr"])
    _assert_equal(got, want, "NaN view")
    assert want["n_points"] > 0 and not (got["src"][:, 0] == 1).any()
    # no hole has a point: NaN, +INF, -1 and masked-out pixels never appear as a source
    for v in (0, 2):
        D, M = depths[v].ravel(), I["masks"][v].ravel()
        px = got["src"][got["src"][:, 0] == v, 1]
        assert np.isfinite(D[px]).all() and (D[px] != -1).all() and (M[px] == 1).all()

    def assert_empty(r):
        assert r["n_points"] == 0 and hip_ctx.mvs_fused_count() == 0
        assert all(r[k].shape[0] == 0 for k in ARRAYS)
        lib = capi.lib()
        assert lib.srh_mvs_fused_download(hip_ctx._h, 0, 0, None, None, None, None, None, None) == capi.SRH_OK
        assert hip_ctx.mvs_fused_download(0, 0)["xyz"].shape == (0, 3)
        assert all(q == 0 for q in hip_ctx.mvs_fused_device().values())
    # the empty view alone
    r = hip_ctx.mvs_fuse([1], p, capi.fuse_params(min_views=1))
    assert r["n_candidates"] == 0
    assert_empty(r)
    # a threshold nothing meets
    r = hip_ctx.mvs_fuse(list(range(n)), p, capi.fuse_params(dist_threshold=1e-12))
    assert r["n_candidates"] > 0 and r["n_unsupported"] == r["n_candidates"] and r["n_claimed"] == 0
    assert_empty(r)


def test_pipeline_estimate_cross_check_fuse(hip_ctx):
    case = cases.get_mvs("mvs_five_views")
    imgs, ocams, op = cases.oracle_inputs(case)
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    n = len(cams)
    neigh = capi.mvs_neighbours(cams, p)
    for v in range(n):
        hip_ctx.mvs_initial_estimate(v, neigh[v], p)
    for v in range(n):
        hip_ctx.mvs_cross_check(list(range(n)), v, p)
    before = [hip_ctx.download_depth(v) for v in range(n)]
    got = hip_ctx.mvs_fuse(list(range(n)), p)                          # threshold: p.cross_check_threshold
    after = [hip_ctx.download_depth(v) for v in range(n)]
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    rgbas = [v[0] for v in case["views"]]
    masks = [v[1] for v in case["views"]]
    want = F.fuse(ocams, op, rgbas, masks, before, op.cross_check_threshold)
    print("pipeline: %s member margin %.3g orientation margin %.3g"
          % ({k: want[k] for k in COUNTERS}, want["member_margin"], want["orient_margin"]))
    assert want["n_points"] > 0
    _assert_equal(got, want, "pipeline")


def test_repeatable_windowed_and_profiled(hip_ctx):
    I = F.case_inputs("mvs_mixed_sizes")
    n = len(I["ocams"])
    p = _upload(hip_ctx, I)
    f = capi.fuse_params(dist_threshold=I["thr"])
    hip_ctx.profile_enable(True)
    hip_ctx.profile_reset()
    try:
        a = hip_ctx.mvs_fuse(list(range(n)), p, f)
        prof = hip_ctx.profile()
    finally:
        hip_ctx.profile_enable(False)
    assert prof["point_cloud_kernel"][1] == n
    for k in ("fuse_view_kernel", "fuse_scan_kernel", "fuse_scatter_kernel"):
        assert prof[k][1] == n, k
    b = hip_ctx.mvs_fuse(list(range(n)), p, f)
    for k in ARRAYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert all(a[k] == b[k] for k in COUNTERS)
    # a later upload does not touch the result
    hip_ctx.upload_depth(0, np.full_like(I["depths"][0], np.nan))
    total = hip_ctx.mvs_fused_count()
    assert total == a["n_points"] > 10
    cuts = [0, 1, 7, total // 2, total - 1, total, total]
    parts = [hip_ctx.mvs_fused_download(lo, hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
    for k in ARRAYS:
        assert np.concatenate([q[k] for q in parts]).tobytes() == a[k].tobytes(), k
    dev = hip_ctx.mvs_fused_device()
    assert all(dev[k] for k in ARRAYS)
    for first, count in ((-1, 1), (0, total + 1), (total, 1), (1, -1), (total + 1, 0)):
        with pytest.raises(capi.StereoHipError) as e:
            hip_ctx.mvs_fused_download(first, count)
        assert e.value.code == capi.SRH_E_INVALID


def test_argument_errors_and_cancellation():
    I = F.case_inputs("mvs_scaled")
    with capi.Context(0) as ctx:
        with pytest.raises(capi.StereoHipError) as e:
            ctx.mvs_fused_count()                                      # nothing fused yet
        assert e.value.code == capi.SRH_E_INVALID
        p = _upload(ctx, I)
        bad = [([0, 1, 0], None), ([0, 5], None), ([], None), ([0, 1], capi.fuse_params(min_views=0))]
        for slots, f in bad:
            with pytest.raises(capi.StereoHipError) as e:
                ctx.mvs_fuse(slots, p, f)
            assert e.value.code == capi.SRH_E_INVALID, slots
        flag = C.c_int(1)
        ctx.set_hooks(flag, None)
        try:
            with pytest.raises(capi.StereoHipError) as e:
                ctx.mvs_fuse([0, 1, 2], p)
            assert e.value.code == capi.SRH_E_CANCELLED
        finally:
            ctx.set_hooks(None, None)
        with pytest.raises(capi.StereoHipError):
            ctx.mvs_fused_count()                                      # a cancelled call leaves no result
        got = ctx.mvs_fuse([0, 1, 2], p, capi.fuse_params(dist_threshold=I["thr"]))
        _assert_equal(got, F.case_result("mvs_scaled"), "after cancellation")
