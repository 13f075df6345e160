"""The support-weighted census cost on the device (option "cost" = COST_CENSUS, srh_view_census, srh_twoview_pair_costs
kind 3, the host class's setCostFunction / cost_census; csrc/srh_census.hip) against its CPU restatement
(tests/census_restatement.cpp, itself held against a numpy statement in tests/test_census_host.py).

Signature planes and depth maps are compared bit for bit, NaN and inf positions included.  Single costs of
srh_twoview_pair_costs have the same special values in the same places and finite values within 8 units in the last
place, the SAD tests' bound for the SAD tests' reason: the device builds its windows with the ROCm device library's exp,
the restatement with sro_weights (the host libm's exp).  wta_margin (1e-10) absorbs those differences in the maps."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import cases
import census_ref as CR
import filter_ref as F
import oracle_ffi as O
import sad_ref as S
import sgm_ref as G
import small_shapes as SS
import subpixel_ref as SR
import test_gpu_host_api as HA
import test_gpu_sad as TS
import test_gpu_subpixel as SP
import test_gpu_wta_outputs as WO
import wide_shapes as WS
from stereoreconstruction_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECTIONS = ((0, 1), (1, 0))
_options, _assert_same, _assert_costs, _case = TS._options, TS._assert_same, TS._assert_costs, TS._case


def _restated_maps(imgs, ocams, op):
    return [CR.twoview_wta_census(imgs[r], imgs[o], ocams[r], ocams[o], op) for r, o in DIRECTIONS]


def _same_words(got, want, tag):
    bad = np.argwhere(got != want)
    assert got.dtype == np.uint64 and got.shape == want.shape and len(bad) == 0, \
        "%s: %d signatures differ, first (y, x) = %s: %#x / %#x" % (tag, len(bad), bad[:3].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


# ---------------------------------------------------------------------------------------------- 1. signatures
@pytest.mark.parametrize("name", ["geodesic_rect", "adaptive_masks", "geodesic_r2"])
def test_view_census_equals_the_restatement(hip_ctx, name):
    case, imgs, ocams, op, cams, p = _case(name)
    cases.upload_case(hip_ctx, case, cams)
    for slot in (0, 1):
        got = hip_ctx.view_census(slot)
        _same_words(got, CR.census_plane(imgs[slot]), "%s slot %d" % (name, slot))
        assert not (got & np.uint64((1 << 31) | (1 << 63))).any() and got.any()


@pytest.mark.parametrize("w,h", [(1, 1), (5, 5), (9, 1), (33, 9), (70, 17)])
def test_view_census_small_views_and_after_a_new_upload(hip_ctx, w, h):
    """views smaller than the 9x7 neighbourhood and its tile, more than one tile; a different image uploaded to the same
    slot gives that image's plane (the cached one is dropped)"""
    K = np.array([[float(max(w, h)), 0, w / 2.0], [0, float(max(w, h)), h / 2.0], [0, 0, 1.0]])
    cam = capi.camera_from_krt(K, np.eye(3), np.zeros(3), None)
    rng = np.random.default_rng(w * 100 + h)
    planes = []
    for k in range(2):
        rgba = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        mask = (rng.random((h, w)) < 0.8).astype(np.uint8)
        hip_ctx.upload_view(0, rgba, mask, cam)
        got = hip_ctx.view_census(0)
        _same_words(got, CR.census_plane(O.OImage(rgba, mask)), "%dx%d upload %d" % (w, h, k))
        _same_words(hip_ctx.view_census(0), got, "%dx%d upload %d, asked again" % (w, h, k))
        planes.append(got)
    if w * h > 1:
        assert not np.array_equal(planes[0], planes[1])


# ---------------------------------------------------------------------------------------------- 2. pair costs
@pytest.mark.parametrize("name", ["geodesic_masks", "adaptive_masks", "geodesic_r2"])
def test_pair_costs_against_the_restatement(hip_ctx, name):
    case, imgs, ocams, op, cams, p = _case(name)
    cases.upload_case(hip_ctx, case, cams)
    h, w = case["views"][0][0].shape[:2]
    xy = TS._pairs(np.random.default_rng(0xCE45 + len(name)), w, h)
    for ref, oth in DIRECTIONS:
        got = hip_ctx.twoview_pair_costs(ref, oth, p, xy, capi.COST_CENSUS)
        want = CR.pair_costs_census(imgs[ref], imgs[oth], op, xy)
        _assert_costs(got, want, "%s census %d>%d" % (name, ref, oth))
        assert (want == op.bad_ret).any() and (want < op.bad_ret).sum() > len(xy) // 2
        assert (got[got != op.bad_ret] >= 0).all() and (got[got != op.bad_ret] <= 62).all()
        again = hip_ctx.twoview_pair_costs(ref, oth, p, xy, capi.COST_CENSUS)
        _assert_same(again, got, "%s census repeat" % name)


# ---------------------------------------------------------------------------------------------- 3. WTA maps, every path
PATHS = TS.PATHS


def _check_paths(hip_ctx, case, imgs, ocams, op, cams, p, want=None):
    cases.upload_case(hip_ctx, case, cams)
    want = want if want is not None else _restated_maps(imgs, ocams, op)
    for tag, opts in PATHS:
        with _options(hip_ctx, cost=capi.COST_CENSUS, **opts):
            for ref, oth in DIRECTIONS:
                hip_ctx.twoview_wta(ref, oth, p)
                assert not hip_ctx.stats()["used_dense_path"]
                _assert_same(hip_ctx.download_depth(ref), want[ref], "%s %s %d>%d" % (case["name"], tag, ref, oth))
    return want


@pytest.mark.parametrize("name", sorted(cases.TWOVIEW_CASES))
def test_wta_every_case_three_paths(hip_ctx, name):
    case, imgs, ocams, op, cams, p = _case(name)
    want = _check_paths(hip_ctx, case, imgs, ocams, op, cams, p)
    assert np.isfinite(want[0]).any()


# (w, h, D, masks, verged): smaller than the window, than a wave tile, more candidates than columns, the tile edges
SMALL = [(1, 1, 2, False, False), (9, 1, 4, False, False), (5, 5, 3, False, False), (8, 8, 6, False, False),
         (33, 9, 40, False, False), (33, 9, 40, True, False), (65, 12, 8, False, False), (65, 12, 8, False, True),
         (40, 3, 64, False, False), (31, 5, 12, False, False), (32, 5, 12, False, False), (33, 5, 12, False, False)]


@pytest.mark.parametrize("radius,kind", SS.TWOVIEW_KINDS, ids=["r5-geodesic", "r2-adaptive"])
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: SS.shape_id(s[:3]) + ("-masks" if s[3] else "") + ("-verged" if s[4] else ""))
def test_wta_small_shapes(hip_ctx, shape, radius, kind):
    w, h, D, masks, verged = shape
    case = SS.small_twoview(w, h, D, radius, kind, masks=masks, verged=verged)
    imgs, ocams, op = cases.oracle_inputs(case)
    cams, p = cases.hip_inputs(case)
    _check_paths(hip_ctx, case, imgs, ocams, op, cams, p)


def _restated_in_bands(imgs, ocams, op, ref, oth):
    """the restatement's pass, its rows in bands on threads (the C code runs outside the GIL)"""
    bands = WS.row_bands(imgs[ref].h)
    with ThreadPoolExecutor(max_workers=len(bands)) as ex:
        parts = list(ex.map(lambda b: CR.twoview_wta_census(imgs[ref], imgs[oth], ocams[ref], ocams[oth], op, b[0], b[1]), bands))
    depth = parts[0]
    for (a, b), d in list(zip(bands, parts))[1:]:
        depth[a:b] = d[a:b]
    return depth


def test_wta_one_wide_view(hip_ctx):
    """1920 x 24 x 256, geodesic r = 5: 60 window tiles per row, lists of up to 256 candidates, 32 blocks per pixel"""
    case = SS.small_twoview(1920, 24, 256, 5, 1)
    imgs, ocams, op = cases.oracle_inputs(case)
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    with _options(hip_ctx, cost=capi.COST_CENSUS):
        for ref, oth in DIRECTIONS:
            hip_ctx.twoview_wta(ref, oth, p)
            assert not hip_ctx.stats()["used_dense_path"]
            got = hip_ctx.download_depth(ref)
            _assert_same(got, _restated_in_bands(imgs, ocams, op, ref, oth), "wide %d>%d" % (ref, oth))
            assert np.isfinite(got).mean() > 0.2


# ---------------------------------------------------------------------------------------------- 4. compute, bands
def _check_compute(ctx, case, imgs, ocams, op, p, tag, filter_flags=0):
    dl, dr = _restated_maps(imgs, ocams, op)
    dl, dr = O.twoview_cross_check(ocams[0], ocams[1], op, dl, dr)
    if filter_flags:
        dl = F.filter_map(case["views"][0][0], case["views"][0][1], dl, F.oparams(p), filter_flags)
        dr = F.filter_map(case["views"][1][0], case["views"][1][1], dr, F.oparams(p), filter_flags)
    with _options(ctx, cost=capi.COST_CENSUS, filter_invalid=filter_flags):
        gl, gr = ctx.twoview_compute(0, 1, p)
        assert not ctx.stats()["used_dense_path"]
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


@pytest.mark.parametrize("name", ["geodesic_masks", "adaptive_verged"])
def test_band_invariance(hip_ctx, name):
    """a row range gives the whole pass's rows and leaves the others alone; a 1 MB band budget (several bands) the same maps"""
    case, imgs, ocams, op, cams, p = _case(name)
    cases.upload_case(hip_ctx, case, cams)
    want = _restated_maps(imgs, ocams, op)
    h = want[0].shape[0]
    for tag, opts in PATHS[:2]:
        with _options(hip_ctx, cost=capi.COST_CENSUS, **opts):
            for ref, oth in DIRECTIONS:
                hip_ctx.upload_depth(ref, np.full(want[ref].shape, -7.0))
                hip_ctx.twoview_wta(ref, oth, p, 7, 19)
                got = hip_ctx.download_depth(ref)
                _assert_same(got[7:19], want[ref][7:19], "%s %s rows 7..19 %d>%d" % (name, tag, ref, oth))
                assert (got[:7] == -7.0).all() and (got[19:] == -7.0).all()
                try:
                    hip_ctx.set_option("band_budget_mb", 1)
                    hip_ctx.twoview_wta(ref, oth, p)
                    _assert_same(hip_ctx.download_depth(ref), want[ref], "%s %s 1 MB bands %d>%d" % (name, tag, ref, oth))
                finally:
                    hip_ctx.set_option("band_budget_mb", 32768)
    assert h > 19


# ---------------------------------------------------------------------------------------------- 5. the stages downstream
@pytest.mark.parametrize("name", ["geodesic_rect", "adaptive_masks", "adaptive_verged"])
def test_label_costs_are_pair_costs(hip_ctx, name):
    case, imgs, ocams, op, cams, p = _case(name)
    cases.upload_case(hip_ctx, case, cams)
    for ref, oth in DIRECTIONS:
        with _options(hip_ctx, cost=capi.COST_CENSUS):
            cost, pix = hip_ctx.twoview_label_costs(ref, oth, p)
            band, _ = hip_ctx.twoview_label_costs(ref, oth, p, 7, 19, want_pixels=False)
        has = pix[..., 0] != capi.LABEL_PIXEL_NONE
        assert has.any()
        yy, xx, dd = np.nonzero(has)
        xy = np.stack([xx, yy, pix[yy, xx, dd, 0], pix[yy, xx, dd, 1]], 1).astype(np.int32)
        pc = hip_ctx.twoview_pair_costs(ref, oth, p, xy, capi.COST_CENSUS)
        tag = "%s %d>%d" % (name, ref, oth)
        _assert_same(cost[yy, xx, dd], pc, tag + " vs pair costs")
        assert (cost[~has] == (2 * p.window_radius + 1) * p.bad_ret).all(), tag
        _assert_same(band, cost[7:19], tag + " band")
        # (and they are census costs: the restatement's, on a sample)
        sub = np.random.default_rng(len(name)).choice(len(xy), size=min(800, len(xy)), replace=False)
        _assert_costs(pc[sub], CR.pair_costs_census(imgs[ref], imgs[oth], op, xy[sub]), tag + " restatement")


def test_compute_sgm_over_the_census_volume(hip_ctx):
    name = "adaptive_masks"
    case, imgs, ocams, op, cams, p = _case(name)
    cases.upload_case(hip_ctx, case, cams)
    with _options(hip_ctx, cost=capi.COST_CENSUS):
        maps, vols = [], []
        for ref, oth in DIRECTIONS:
            cost, _ = hip_ctx.twoview_label_costs(ref, oth, p, want_pixels=False)
            vols.append(cost)
            maps.append(G.aggregate(cost, view_mask=case["views"][ref][1], min_depth=op.min_depth, max_depth=op.max_depth))
        dl, dr = O.twoview_cross_check(ocams[0], ocams[1], op, maps[0]["depth"], maps[1]["depth"])
        gl, gr, infos = hip_ctx.twoview_compute_sgm(0, 1, p)
        labels, D, sums = hip_ctx.twoview_sgm_state(*hip_ctx.twoview_sgm_dims(), want_costs=True)
    _assert_same(gl, dl, name + " sgm left")
    _assert_same(gr, dr, name + " sgm right")
    assert np.array_equal(labels, maps[1]["labels"]) and S.same_bits(sums, maps[1]["S"]) and S.same_bits(D, vols[1])
    with _options(hip_ctx, cost=capi.COST_SAD):
        sad_vol, _ = hip_ctx.twoview_label_costs(1, 0, p, want_pixels=False)
    assert not S.same_bits(sad_vol, vols[1])


@pytest.mark.parametrize("name", ["geodesic_rect", "geodesic_verged_dist_masks"])
def test_wta_outputs_costs_are_census_pair_costs(hip_ctx, name):
    case, p = WO._setup(hip_ctx, name)
    imgs, ocams, op = cases.oracle_inputs(case)
    for ref, oth in DIRECTIONS:
        with WO._options(hip_ctx, wta_outputs=3, cost=capi.COST_CENSUS):
            depth, planes, st = WO._pass(hip_ctx, ref, oth, p)
        assert not st["used_dense_path"]
        tag = "%s %d>%d" % (name, ref, oth)
        for xy, got in WO._assert_pair_costs(hip_ctx, ref, oth, p, planes, capi.COST_CENSUS, tag):
            _assert_costs(got, CR.pair_costs_census(imgs[ref], imgs[oth], op, xy), tag + " restatement")
        _assert_same(depth, CR.twoview_wta_census(imgs[ref], imgs[oth], ocams[ref], ocams[oth], op), tag + " depth")


def test_subpixel_replay_under_census(hip_ctx):
    case = cases.get_twoview("adaptive_masks")
    p = SP._setup(hip_ctx, case)
    for ref, oth in DIRECTIONS:
        integer, got = SP._integer_and_refined(hip_ctx, p, ref, oth, cost=capi.COST_CENSUS)
        counts = SP._replay(hip_ctx, case, p, ref, oth, got, integer, kind=capi.COST_CENSUS)
        assert counts[SR.REFINED] > 0


# ---------------------------------------------------------------------------------------------- 6. the option
def test_switching_costs_on_one_context(hip_ctx):
    """NCC -> census -> SAD -> NCC on one context and pair: the last NCC maps are the first ones' bits, census and SAD are
    their restatements' (nothing cached for one cost -- the fully-usable-window planes, the learnt list paths, the
    signatures -- leaks into another)"""
    for name in ("geodesic_rect", "adaptive_verged"):
        case, imgs, ocams, op, cams, p = _case(name)
        cases.upload_case(hip_ctx, case, cams)
        ncc1 = hip_ctx.twoview_compute(0, 1, p)
        with _options(hip_ctx, cost=capi.COST_CENSUS):
            census = hip_ctx.twoview_compute(0, 1, p)
        with _options(hip_ctx, cost=capi.COST_SAD):
            sad = hip_ctx.twoview_compute(0, 1, p)
        ncc2 = hip_ctx.twoview_compute(0, 1, p)
        want_c = O.twoview_cross_check(ocams[0], ocams[1], op, *_restated_maps(imgs, ocams, op))
        want_s = O.twoview_cross_check(ocams[0], ocams[1], op, *TS._restated_maps(imgs, ocams, op))
        for k in range(2):
            _assert_same(ncc2[k], ncc1[k], "%s ncc again %d" % (name, k))
            _assert_same(census[k], want_c[k], "%s census %d" % (name, k))
            _assert_same(sad[k], want_s[k], "%s sad %d" % (name, k))
            assert not S.same_bits(census[k], ncc1[k]) and not S.same_bits(census[k], sad[k])


def test_cost_rows_under_census_raises(hip_ctx):
    case, imgs, ocams, op, cams, p = _case("geodesic_rect")
    cases.upload_case(hip_ctx, case, cams)
    for sad_dense in (0, 1):
        with TS._options(hip_ctx, cost=capi.COST_CENSUS):
            try:
                hip_ctx.set_option("sad_dense", sad_dense)
                with pytest.raises(capi.StereoHipError):
                    hip_ctx.twoview_cost_rows(0, 1, p, 0, 4, 0)
                # sad_dense is ignored: the lists take the pass
                hip_ctx.twoview_wta(0, 1, p)
                assert not hip_ctx.stats()["used_dense_path"]
            finally:
                hip_ctx.set_option("sad_dense", 0)
    with pytest.raises(capi.StereoHipError):
        hip_ctx.twoview_pair_costs(0, 1, p, np.array([[1, 1, 1, 1]], np.int32), 2)


# ---------------------------------------------------------------------------------------------- 7. the host class
def test_host_class_census(hip_ctx, tmp_path):
    subprocess.check_call(["make", "-C", HA.HOST], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "host_census_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + HA.HOST,
                           os.path.join(ROOT, "tests", "host_census_test.cpp"),
                           os.path.join(HA.HOST, "libstereo_recon_host.a"),
                           "-L" + HA.LIBDIR, "-lstereo_recon_hip", "-Wl,-rpath," + HA.LIBDIR, "-o", exe])
    case = cases.get_twoview("geodesic_masks")
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    with _options(hip_ctx, cost=capi.COST_CENSUS):
        want = hip_ctx.twoview_compute(0, 1, p)
    h, w = want[0].shape
    inp = str(tmp_path / "in.bin")
    HA._write_input(inp, case, True)
    outp = str(tmp_path / "out.bin")
    subprocess.check_call([exe, "compute", inp, outp, str(capi.COST_CENSUS)])
    (gl, gr), steps = HA._read_output(outp, 2, w, h)
    assert steps == [1, 3, 5, 8]
    _assert_same(gl, want[0], "host left")
    _assert_same(gr, want[1], "host right")
    xy = np.array([[5, 5, 9, 5], [w - 1, h - 1, w - 1, h - 1], [20, 17, 3, 30], [0, 0, -2, 1]], np.int32)
    outp2 = str(tmp_path / "pairs.bin")
    subprocess.check_call([exe, "pairs", inp, outp2] + [str(v) for v in xy.reshape(-1)])
    got = np.fromfile(outp2, np.float64).reshape(-1, 2)
    _assert_same(got[:, 0], hip_ctx.twoview_pair_costs(0, 1, p, xy, capi.COST_CENSUS), "host cost_census")
    _assert_same(got[:, 1], hip_ctx.twoview_pair_costs(0, 1, p, xy, capi.COST_SAD), "host cost_sad")
