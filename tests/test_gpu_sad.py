"""The SAD matching cost on the device (option "cost" = SRH_COST_SAD, srh_twoview_pair_costs, the host class's
setCostFunction / cost_sad) against the CPU restatement of TwoViewStereo::cost_sad and its WTA pass
(tests/sad_restatement.cpp).  Depth maps are compared bit for bit, NaN and inf positions included.  Single costs of
srh_twoview_pair_costs are compared with the same bad_ret / NaN / inf positions and finite values within a few units in the
last place: the device builds its windows with the ROCm device library's exp, the restatement with sro_weights (the host
libm's exp), and the two differ by one unit in the last place on some arguments."""
import contextlib
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import cases
import filter_ref as F
import oracle_ffi as O
import sad_ref as S
import test_gpu_host_api as HA
from stereoreconstruction_amd import capi, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "bunny_pair.npz")


@contextlib.contextmanager
def _options(ctx, **opts):
    """set options on the shared context, and put the defaults back whatever happens"""
    defaults = dict(cost=capi.COST_NCC, list_rows=1, force_generic=0, filter_invalid=0)
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k in opts:
            ctx.set_option(k, defaults[k])


def _assert_same(got, want, tag):
    assert S.same_bits(got, want), "%s: %s" % (tag, S.diff_report(got, want))


def _assert_costs(got, want, tag, ulps=8, rtol=0.0):
    """the same special values in the same places, finite costs within `ulps` units in the last place (or rtol)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(np.isnan(got), np.isnan(want)), tag
    assert np.array_equal(got[~fin], want[~fin]) or np.isnan(want[~fin]).all(), tag
    assert np.array_equal(got == 1000.0, want == 1000.0), tag + ": bad_ret positions"
    tol = np.maximum(ulps * np.spacing(np.abs(want[fin])), rtol * np.maximum(1.0, np.abs(want[fin])))
    bad = np.abs(got[fin] - want[fin]) > tol
    assert not bad.any(), "%s: %d of %d beyond %d ulp" % (tag, bad.sum(), fin.sum(), ulps)


def _case(name):
    case = cases.get_twoview(name)
    imgs, ocams, op = cases.oracle_inputs(case)
    cams, p = cases.hip_inputs(case)
    return case, imgs, ocams, op, cams, p


def _pairs(rng, w, h, n=3000):
    """random pairs plus border, last row / column and out-of-bounds candidates"""
    xy = np.stack([rng.integers(0, w, n), rng.integers(0, h, n), rng.integers(-3, w + 3, n), rng.integers(-3, h + 3, n)], 1)
    edge = []
    for x1, y1 in ((0, 0), (w - 1, h - 1), (w - 1, 0), (0, h - 1), (w - 2, h - 2), (w // 2, h - 1), (w - 1, h // 2)):
        for x2, y2 in ((0, 0), (w - 1, h - 1), (w - 1, y1), (x1, h - 1), (-1, y1), (w, y1), (x1, -6), (x1, h + 5),
                       (w - 2, h - 2), (w // 2, h // 2)):
            edge.append((x1, y1, x2, y2))
    return np.concatenate([xy, np.array(edge)]).astype(np.int32)


@pytest.mark.parametrize("name", ["geodesic_masks", "adaptive_masks", "geodesic_r2"])
def test_pair_costs_against_restatement_and_oracle_ncc(hip_ctx, name):
    case, imgs, ocams, op, cams, p = _case(name)
    cases.upload_case(hip_ctx, case, cams)
    h, w = case["views"][0][0].shape[:2]
    xy = _pairs(np.random.default_rng(0x5AD0 + len(name)), w, h)
    for ref, oth in ((0, 1), (1, 0)):
        got = hip_ctx.twoview_pair_costs(ref, oth, p, xy, capi.COST_SAD)
        want = S.pair_costs_sad(imgs[ref], imgs[oth], op, xy)
        _assert_costs(got, want, "%s sad %d>%d" % (name, ref, oth))
        assert (want == op.bad_ret).any() and (want < op.bad_ret).sum() > len(xy) // 2
        # (deterministic: the same pairs give the same bits)
        again = hip_ctx.twoview_pair_costs(ref, oth, p, xy, capi.COST_SAD)
        _assert_same(again, got, "%s sad repeat" % name)
        got = hip_ctx.twoview_pair_costs(ref, oth, p, xy[:600], capi.COST_NCC)
        _assert_costs(got, S.pair_costs_ncc(imgs[ref], imgs[oth], op, xy[:600]), "%s ncc %d>%d" % (name, ref, oth), rtol=1e-9)


def _restated_maps(imgs, ocams, op):
    return [S.twoview_wta_sad(imgs[r], imgs[o], ocams[r], ocams[o], op) for r, o in ((0, 1), (1, 0))]


PATHS = (("rows", {}), ("list_order", dict(list_rows=0)), ("walk", dict(force_generic=2)))


@pytest.mark.parametrize("name", sorted(cases.TWOVIEW_CASES))
def test_wta_every_case_three_paths(hip_ctx, name):
    case, imgs, ocams, op, cams, p = _case(name)
    cases.upload_case(hip_ctx, case, cams)
    want = _restated_maps(imgs, ocams, op)
    for tag, opts in PATHS:
        with _options(hip_ctx, cost=capi.COST_SAD, **opts):
            for ref, oth in ((0, 1), (1, 0)):
                hip_ctx.twoview_wta(ref, oth, p)
                assert not hip_ctx.stats()["used_dense_path"]
                _assert_same(hip_ctx.download_depth(ref), want[ref], "%s %s %d>%d" % (name, tag, ref, oth))


def _check_compute(ctx, case, imgs, ocams, op, p, tag, filter_flags=0):
    dl, dr = _restated_maps(imgs, ocams, op)
    dl, dr = O.twoview_cross_check(ocams[0], ocams[1], op, dl, dr)
    if filter_flags:
        dl = F.filter_map(case["views"][0][0], case["views"][0][1], dl, F.oparams(p), filter_flags)
        dr = F.filter_map(case["views"][1][0], case["views"][1][1], dr, F.oparams(p), filter_flags)
    with _options(ctx, cost=capi.COST_SAD, filter_invalid=filter_flags):
        gl, gr = ctx.twoview_compute(0, 1, p)
    _assert_same(gl, dl, tag + " left")
    _assert_same(gr, dr, tag + " right")
    return gl, gr


@pytest.mark.parametrize("name", ["geodesic_rect", "adaptive_verged", "geodesic_verged_dist_masks"])
def test_compute_with_cross_check(hip_ctx, name):
    case, imgs, ocams, op, cams, p = _case(name)
    cases.upload_case(hip_ctx, case, cams)
    gl, gr = _check_compute(hip_ctx, case, imgs, ocams, op, p, name)
    assert np.isfinite(gl).sum() > 0 and np.isinf(gl).sum() + np.isnan(gl).sum() > 0
    if name == "geodesic_rect":
        _check_compute(hip_ctx, case, imgs, ocams, op, p, name + " filtered", capi.FILTER_GAPS | capi.FILTER_MEDIAN)


def _load_bunny():
    g = np.load(GOLD)
    views = []
    for tag in ("left", "right"):
        views.append((g[tag + "_rgba"], g[tag + "_mask"], (g[tag + "_K"], g[tag + "_R"], g[tag + "_t"]),
                      g[tag + "_dist"], None))
    params = dict(min_depth=30.0, max_depth=80.0, num_depth_levels=100, image_scale=float(g["scale"][0]),
                  window_radius=5, weight_kind=1)
    return dict(name="bunny", kind="twoview", views=views, params=params)


def test_bunny_pair_whole_maps(hip_ctx):
    case = _load_bunny()
    imgs, ocams, op = cases.oracle_inputs(case)
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    gl, gr = _check_compute(hip_ctx, case, imgs, ocams, op, p, "bunny")
    assert np.isfinite(gl).sum() > 1000 and np.isfinite(gr).sum() > 1000


def _rows(H, R=5):
    """8 stratified rows: the first and last, the rows either side of where windows stop crossing the border, interior"""
    rows = [0, R - 1, R, H // 3, H // 2 + 7, H - R - 1, H - R, H - 1]
    assert len(set(rows)) == 8
    return rows


@pytest.mark.parametrize("geometry", ["c3_rectified", "c5_refractive"])
def test_full_size_stratified_rows(hip_ctx, geometry):
    W, H, D = 1920, 1080, 256
    seed = 0x5EED0003 if geometry == "c3_rectified" else 0x5EED0050
    L, R, ml, mr, _ = synthetic.rectified_pair(W, H, D, seed)
    (Kl, Rl, tl), (Kr, Rr, tr) = synthetic.rectified_cameras(W, H)
    zmin, zmax = synthetic.rectified_depth_range(W, D)
    plane = (np.array([0.0, 0.0, 1.0]), 0.1, 1.333) if geometry == "c5_refractive" else (None, 0.0, 1.0)
    hip_ctx.upload_view(0, L, ml, capi.camera_from_krt(Kl, Rl, tl, None, *plane))
    hip_ctx.upload_view(1, R, mr, capi.camera_from_krt(Kr, Rr, tr, None, *plane))
    kw = dict(min_depth=zmin, max_depth=zmax, num_depth_levels=D, weight_kind=capi.WEIGHT_GEODESIC)
    p = capi.params_twoview(**kw)
    op = O.params_twoview(**kw)
    oc = [O.camera_set(Kl, Rl, tl, None, *plane), O.camera_set(Kr, Rr, tr, None, *plane)]
    oi = [O.OImage(L, ml), O.OImage(R, mr)]
    rows = _rows(H)
    got = []
    with _options(hip_ctx, cost=capi.COST_SAD):
        for ref, oth in ((0, 1), (1, 0)):
            hip_ctx.twoview_wta(ref, oth, p)
            assert not hip_ctx.stats()["used_dense_path"]
            got.append(hip_ctx.download_depth(ref))
    for ref, oth in ((0, 1), (1, 0)):
        with ThreadPoolExecutor(max_workers=8) as ex:
            want = list(ex.map(lambda y: S.twoview_wta_sad(oi[ref], oi[oth], oc[ref], oc[oth], op, y, y + 1)[y], rows))
        for y, wrow in zip(rows, want):
            _assert_same(got[ref][y], wrow, "%s %d>%d row %d" % (geometry, ref, oth, y))
        assert np.isfinite(got[ref]).mean() > 0.2


def test_switching_costs_on_one_context(hip_ctx):
    """NCC -> SAD -> NCC on the same context and views: the NCC maps keep their bits both times (nothing cached for one
    cost -- the fully-usable-window planes, the learnt list paths -- leaks into the other), and SAD differs from NCC."""
    for name in ("geodesic_rect", "adaptive_verged"):
        case, imgs, ocams, op, cams, p = _case(name)
        cases.upload_case(hip_ctx, case, cams)
        ncc1 = hip_ctx.twoview_compute(0, 1, p)
        with _options(hip_ctx, cost=capi.COST_SAD):
            sad = hip_ctx.twoview_compute(0, 1, p)
        ncc2 = hip_ctx.twoview_compute(0, 1, p)
        for k in range(2):
            _assert_same(ncc2[k], ncc1[k], "%s ncc again %d" % (name, k))
            assert not S.same_bits(sad[k], ncc1[k])
        want = O.twoview_cross_check(ocams[0], ocams[1], op, *(O.twoview_wta(imgs[r], imgs[o], ocams[r], ocams[o], op)
                                                              for r, o in ((0, 1), (1, 0))))
        for k in range(2):
            ok, msg, _ = cases.compare_depth(ncc1[k], want[k], 1e-9)
            assert ok, (name, k, msg)


def test_cost_option_values(hip_ctx):
    with pytest.raises(capi.StereoHipError):
        hip_ctx.set_option("cost", 2)
    case, imgs, ocams, op, cams, p = _case("geodesic_rect")
    cases.upload_case(hip_ctx, case, cams)
    with _options(hip_ctx, cost=capi.COST_SAD):
        with pytest.raises(capi.StereoHipError):
            hip_ctx.twoview_cost_rows(0, 1, p, 0, 4, 0)


def test_host_class_sad(hip_ctx, tmp_path):
    subprocess.check_call(["make", "-C", HA.HOST], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "host_sad_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + HA.HOST,
                           os.path.join(ROOT, "tests", "host_sad_test.cpp"),
                           os.path.join(HA.HOST, "libstereo_recon_host.a"),
                           "-L" + HA.LIBDIR, "-lstereo_recon_hip", "-Wl,-rpath," + HA.LIBDIR, "-o", exe])
    case = cases.get_twoview("geodesic_masks")
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    with _options(hip_ctx, cost=capi.COST_SAD):
        want = hip_ctx.twoview_compute(0, 1, p)
    h, w = want[0].shape
    inp = str(tmp_path / "in.bin")
    HA._write_input(inp, case, True)
    outp = str(tmp_path / "out.bin")
    subprocess.check_call([exe, "compute", inp, outp, str(capi.COST_SAD)])
    (gl, gr), steps = HA._read_output(outp, 2, w, h)
    assert steps == [1, 3, 5, 8]
    _assert_same(gl, want[0], "host left")
    _assert_same(gr, want[1], "host right")
    # the protected costs of a subclass: the C-ABI's pair costs
    xy = np.array([[5, 5, 9, 5], [w - 1, h - 1, w - 1, h - 1], [20, 17, 3, 30], [0, 0, -2, 1]], np.int32)
    outp2 = str(tmp_path / "pairs.bin")
    subprocess.check_call([exe, "pairs", inp, outp2] + [str(v) for v in xy.reshape(-1)])
    got = np.fromfile(outp2, np.float64).reshape(-1, 2)
    _assert_same(got[:, 0], hip_ctx.twoview_pair_costs(0, 1, p, xy, capi.COST_SAD), "host cost_sad")
    _assert_same(got[:, 1], hip_ctx.twoview_pair_costs(0, 1, p, xy, capi.COST_NCC), "host cost_ncc")
