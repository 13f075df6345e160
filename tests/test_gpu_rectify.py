"""Rectification on the GPU (srh_view_rectify_map, srh_twoview_rectify, srh_view_depth_unrectify) against the
numpy reference tests/rectify_ref.py: the map within the parity tolerance 1e-9, the warped bytes and mask bit for bit on the
device's own map, the slot a rectify leaves, the example project's pair on the dense plan against the oracle, and the depth
maps' way back into the views the user handed in."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cases
import oracle_ffi as O
import rectify_ref as R
import test_gpu_host_api as HA
from stereoreconstruction_amd import capi, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9


@pytest.fixture(scope="module")
def small():
    case = R.small_case()
    cams, p = cases.hip_inputs(case)
    return case, cams, p


@pytest.fixture(scope="module")
def bunny():
    case = R.bunny_case()
    cams, p = cases.hip_inputs(case)
    return case, cams, p


def _upload(ctx, case, cams):
    cases.upload_case(ctx, case, cams)
    return [(v[0], v[1]) for v in case["views"]]


def _close(got, want):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = ~np.isnan(want)
    assert (np.abs(got[fin] - want[fin]) <= TOL * (1 + np.abs(want[fin]))).all()
    return fin


@pytest.mark.parametrize("size", [(67, 35), (1, 1), (64, 1), (130, 3)], ids=lambda s: "%dx%d" % s)
def test_map(hip_ctx, small, size):
    case, cams, p = small
    _upload(hip_ctx, case, cams)
    ow, oh = size
    ra, rb = capi.rectify_cameras(cams[0], cams[1], 61, 47, p.image_scale, capi.rectify_params(out_w=ow, out_h=oh))
    for slot, rect in ((0, ra), (1, rb)):
        got = hip_ctx.rectify_map(slot, rect, ow, oh, p.image_scale)
        fin = _close(got, R.warp_map(rect, cams[slot], ow, oh, p.image_scale))
        assert fin.all()                                  # (nothing of these views lies behind its source)
    # a rectified camera turned away: every pixel behind the source, NaN in both
    K, Rm = R.cam_K(ra), R.cam_R(ra)
    away = capi.camera_from_krt(K, cases._rot_y(np.pi) @ Rm, -(cases._rot_y(np.pi) @ Rm) @ R.cam_C(ra))
    got = hip_ctx.rectify_map(0, away, ow, oh, p.image_scale)
    assert np.isnan(got).all() and np.isnan(R.warp_map(away, cams[0], ow, oh, p.image_scale)).all()


def test_bytes_and_mask(hip_ctx, small):
    case, cams, p = small
    src = _upload(hip_ctx, case, cams)
    ow, oh = 67, 35
    r = capi.rectify_params(out_w=ow, out_h=oh)
    rect = capi.rectify_cameras(cams[0], cams[1], 61, 47, p.image_scale, r)
    maps = [hip_ctx.rectify_map(s, rect[s], ow, oh, p.image_scale) for s in (0, 1)]
    info = hip_ctx.twoview_rectify(0, 1, 2, 3, p, r)
    fresh = []
    for s in (0, 1):
        want_rgba, want_mask = R.bilinear(src[s][0], src[s][1], maps[s])
        assert 0.05 <= want_mask.mean() <= 0.95
        rgba, mask = hip_ctx.download_view_image(2 + s)
        assert rgba.shape == (oh, ow, 4)
        assert np.array_equal(rgba, want_rgba) and np.array_equal(mask, want_mask)
        assert info["white_a" if s == 0 else "white_b"] == int(want_mask.sum())
        fresh.append((rgba, mask))
    assert info["fx_bx"] > 0
    for s, key in ((0, "angle_a"), (1, "angle_b")):
        want = np.arccos(np.clip(R.cam_R(cams[s])[2] @ R.cam_R(rect[s])[2], -1, 1))
        assert abs(info[key] - want) <= TOL and 0 < info[key] < 0.2
    # dst == src: the same bytes
    hip_ctx.twoview_rectify(0, 1, 0, 1, p, r)
    for s in (0, 1):
        rgba, mask = hip_ctx.download_view_image(s)
        assert np.array_equal(rgba, fresh[s][0]) and np.array_equal(mask, fresh[s][1])
    # ... and swapped destinations read the sources, not each other's results
    _upload(hip_ctx, case, cams)
    hip_ctx.twoview_rectify(0, 1, 1, 0, p, r)
    for s in (0, 1):
        rgba, mask = hip_ctx.download_view_image(1 - s)
        assert np.array_equal(rgba, fresh[s][0]) and np.array_equal(mask, fresh[s][1])


@pytest.mark.parametrize("seed", [0x5EED0E11, 0x5EED0E12])
def test_identity(hip_ctx, seed):
    """An already rectified pair through the warp: bytes identical, mask identical inside the one-pixel frame, and the
    depth maps of srh_twoview_compute equal to the unrectified run's wherever both masks are WHITE.  (The last part holds
    only because the map snaps to whole pixels and a tap of weight 0 is not asked for support: with the last column and row
    not WHITE, 2 to 39 of the 780 pixels matched differently near them.)"""
    w, h, D = 65, 12, 8
    L, Rr, ml, mr, _ = synthetic.rectified_pair(w, h, D, seed)
    ckrt = synthetic.rectified_cameras(w, h)
    zmin, zmax = synthetic.rectified_depth_range(w, D)
    case = dict(name="identity", kind="twoview", views=[(L, ml, ckrt[0], None, None), (Rr, mr, ckrt[1], None, None)],
                params=dict(min_depth=zmin, max_depth=zmax, num_depth_levels=D, window_radius=2, weight_kind=1, image_scale=1.0))
    cams, p = cases.hip_inputs(case)
    src = _upload(hip_ctx, case, cams)
    plain = hip_ctx.twoview_compute(0, 1, p)
    assert hip_ctx.stats()["used_dense_path"]
    r = capi.rectify_params(flags=capi.RECTIFY_SHARED_CX, focal=float(w), cx_a=w / 2.0, cx_b=w / 2.0, cy=h / 2.0)
    hip_ctx.twoview_rectify(0, 1, 2, 3, p, r)
    masks = []
    for s in (0, 1):
        rgba, mask = hip_ctx.download_view_image(2 + s)
        assert np.array_equal(rgba, src[s][0])
        assert np.array_equal(mask[1:-1, 1:-1], src[s][1][1:-1, 1:-1])
        masks.append(mask)
    rect = hip_ctx.twoview_compute(2, 3, p)
    assert hip_ctx.stats()["used_dense_path"]
    for s in (0, 1):
        both = (masks[s] == 1) & (src[s][1] == 1)
        ok, msg, _ = cases.compare_depth(np.where(both, rect[s], np.nan), np.where(both, plain[s], np.nan), TOL)
        assert ok, msg
        assert np.isfinite(plain[s][both]).sum() > 100


def test_slot_state(hip_ctx, small):
    case, cams, p = small
    src = _upload(hip_ctx, case, cams)
    hip_ctx.set_option("wta_outputs", capi.WTA_WINNERS)
    try:
        hip_ctx.upload_view(2, src[0][0], src[0][1], cams[0])
        hip_ctx.upload_view(3, src[1][0], src[1][1], cams[1])
        hip_ctx.twoview_wta(2, 3, p)
        assert hip_ctx.wta_outputs_state(2)[0] == capi.WTA_WINNERS and np.isfinite(hip_ctx.download_depth(2)).any()
        hip_ctx.twoview_rectify(0, 1, 2, 3, p, capi.rectify_params(out_w=67, out_h=35))
    finally:
        hip_ctx.set_option("wta_outputs", 0)
    for s in (2, 3):
        assert hip_ctx.view_size(s) == (67, 35)
        assert np.isnan(hip_ctx.download_depth(s)).all()
        assert hip_ctx.wta_outputs_state(s)[0] == 0
    assert hip_ctx.view_size(0) == (61, 47)
    # a refused call: a refractive source
    K, Rm, t = case["views"][1][2]
    wet = capi.camera_from_krt(K, Rm, t, None, np.array([0.0, 0.0, 1.0]), 0.1, 1.333)
    hip_ctx.upload_view(5, src[1][0], src[1][1], wet)
    probe = capi.rectify_cameras(cams[0], cams[1], 61, 47, p.image_scale)[0]
    slots = (0, 5, 2, 3)
    before = [hip_ctx.download_view_image(s) for s in slots]
    maps = [hip_ctx.rectify_map(s, probe, 16, 8) for s in (0, 2, 3)]           # what a slot's camera makes of a fixed probe
    with pytest.raises(capi.StereoHipError) as e:
        hip_ctx.twoview_rectify(0, 5, 2, 3, p)
    assert e.value.code == capi.SRH_E_UNSUPPORTED
    with pytest.raises(capi.StereoHipError) as e:
        hip_ctx.twoview_rectify(0, 0, 2, 3, p)
    assert e.value.code == capi.SRH_E_INVALID
    with pytest.raises(capi.StereoHipError) as e:
        hip_ctx.twoview_rectify(0, 64, 2, 3, p)                                    # no such slot (the session's context may hold views anywhere)
    assert e.value.code == capi.SRH_E_INVALID
    for s, (rgba, mask) in zip(slots, before):
        now = hip_ctx.download_view_image(s)
        assert np.array_equal(now[0], rgba) and np.array_equal(now[1], mask)
    for s, m in zip((0, 2, 3), maps):
        assert np.array_equal(hip_ctx.rectify_map(s, probe, 16, 8), m, equal_nan=True)
    with pytest.raises(capi.StereoHipError) as e:
        hip_ctx.rectify_map(5, probe, 16, 8)
    assert e.value.code == capi.SRH_E_UNSUPPORTED


def _ocam(cam):
    return O.camera_set(R.cam_K(cam), R.cam_R(cam), np.array(cam.t))


def test_bunny_rectified_wta_band_runs_the_dense_plan(hip_ctx, bunny):
    case, cams, p = bunny
    src = _upload(hip_ctx, case, cams)
    h, w = src[0][1].shape
    info = hip_ctx.twoview_rectify(0, 1, 2, 3, p)
    print("rectify info", info, "source WHITE", [int(s[1].sum()) for s in src])
    assert info["white_a"] >= 0.8 * src[0][1].sum() and info["white_b"] >= 0.8 * src[1][1].sum()
    rect = capi.rectify_cameras(cams[0], cams[1], w, h, p.image_scale)
    assert capi.twoview_row_aligned(rect[0], rect[1])[0]
    views = [hip_ctx.download_view_image(s) for s in (2, 3)]
    best = int(np.argmax((views[0][1] == 1).sum(axis=1)))
    y0 = min(max(best - 12, 0), h - 24)
    y1 = y0 + 24
    imgs = [O.OImage(v[0], v[1]) for v in views]
    ocams = [_ocam(c) for c in rect]
    op = O.params_twoview(**case["params"])
    want = [O.twoview_wta(imgs[0], imgs[1], ocams[0], ocams[1], op, y0, y1),
            O.twoview_wta(imgs[1], imgs[0], ocams[1], ocams[0], op, y0, y1)]
    # The plan is the dense one under the default options.  Its cost kernel is the persistent strip form only for bands of
    # 24 576 tiles and more (a 256-column band of 24 rows has 192: the driver takes the per-tile kernel, same bits), so the
    # strip kernel is asked for by option "strip" = 8, as tests/test_gpu_strip.py does.
    try:
        for strip in (1, 8):
            hip_ctx.set_option("strip", strip)
            for k, (ref, oth) in enumerate(((2, 3), (3, 2))):
                hip_ctx.upload_depth(ref, np.full((h, w), np.nan))
                hip_ctx.twoview_wta(ref, oth, p, y0, y1)
                st = hip_ctx.stats()
                print("strip", strip, "pass", ref, oth, {n: st[n] for n in ("used_dense_path", "used_strip_kernel", "n_pixels", "n_certified",
                                                                            "n_flagged", "scan_tiles_template", "scan_tiles_walked")})
                assert st["used_dense_path"] == 1
                if strip == 8:
                    assert st["used_strip_kernel"] == 1
                ok, msg, _ = cases.compare_depth(hip_ctx.download_depth(ref)[y0:y1], want[k][y0:y1], TOL)
                assert ok, "strip %d, %s: %s" % (strip, ("left", "right")[k], msg)
    finally:
        hip_ctx.set_option("strip", 1)
    for wnt in want:
        assert np.isfinite(wnt[y0:y1]).sum() > 200


def test_bunny_full_compute_and_back(hip_ctx, bunny):
    case, cams, p = bunny
    src = _upload(hip_ctx, case, cams)
    hip_ctx.twoview_rectify(0, 1, 2, 3, p)
    hip_ctx.twoview_compute(2, 3, p)
    assert hip_ctx.stats()["used_dense_path"] == 1
    hip_ctx.depth_unrectify(2, 0, p)
    hip_ctx.depth_unrectify(3, 1, p)
    left, right = hip_ctx.download_depth(0), hip_ctx.download_depth(1)
    assert left.shape == src[0][1].shape
    fin = np.isfinite(left)
    print("finite left depths", int(fin.sum()), "median", float(np.median(left[fin])), "right", int(np.isfinite(right).sum()))
    assert 38 < np.median(left[fin]) < 48                       # the bunny sits at z ~ 41-44 (tests/test_gpu_bunny.py)
    assert np.isnan(left[src[0][1] != 1]).all() and np.isfinite(right).sum() > 1000


def _rectified_small(hip_ctx, small):
    case, cams, p = small
    src = _upload(hip_ctx, case, cams)
    r = capi.rectify_params(out_w=67, out_h=35)
    hip_ctx.twoview_rectify(0, 1, 2, 3, p, r)
    rect = capi.rectify_cameras(cams[0], cams[1], 61, 47, p.image_scale, r)
    return src, cams, p, rect


def test_unrectify(hip_ctx, small):
    src, cams, p, rect = _rectified_small(hip_ctx, small)
    rw, rh, w, h = 67, 35, 61, 47
    rng = np.random.default_rng(5)
    dr = rng.uniform(8.0, 60.0, (rh, rw))
    yy, xx = np.mgrid[0:rh, 0:rw]
    k = (xx + 3 * yy) % 11
    dr[k == 0], dr[k == 1], dr[k == 2] = np.inf, np.nan, -1.0
    hip_ctx.upload_depth(2, dr)
    idx = hip_ctx.depth_unrectify(2, 0, p, want_index=True)
    got = hip_ctx.download_depth(0)
    x2, y2, inside, csrc, dirs = R.unrectify_coords(cams[0], rect[0], w, h, rw, rh, p.image_scale)
    white = src[0][1] == 1
    sure = (np.abs(x2 - np.round(x2)) > 1e-6) & (np.abs(y2 - np.round(y2)) > 1e-6)
    assert (~sure).mean() <= 0.005
    want_idx = np.where(inside & white, np.trunc(y2) * rw + np.trunc(x2), -1).astype(np.int64)
    assert np.array_equal(idx[sure], want_idx[sure])
    assert (idx[~white] == -1).all() and 0.2 < (idx >= 0).mean() < 0.95 and (idx[white] == -1).any()
    assert idx.max() < rw * rh
    # the depths: the stated formula at the device's own index
    assert np.isnan(got[idx < 0]).all()
    hit = idx >= 0
    read = dr.reshape(-1)[idx[hit]]
    plain = np.isfinite(read) & (read > 0)
    want = R.unrectify_depth(cams[0], rect[0], csrc, dirs[hit][plain], read[plain])
    assert (np.abs(got[hit][plain] - want) <= TOL * np.abs(want)).all() and plain.sum() > 500
    through = got[hit][~plain]
    assert np.array_equal(through.view(np.uint64), read[~plain].view(np.uint64))
    assert np.isposinf(through).any() and np.isnan(through).any() and (through == -1.0).any()
    # a rectified view whose centre is somewhere else
    K, Rm = R.cam_K(rect[0]), R.cam_R(rect[0])
    moved = capi.camera_from_krt(K, Rm, -Rm @ (R.cam_C(rect[0]) + np.array([1e-6, 0.0, 0.0])))
    rgba, mask = hip_ctx.download_view_image(2)
    hip_ctx.upload_view(4, rgba, mask, moved)
    with pytest.raises(capi.StereoHipError) as e:
        hip_ctx.depth_unrectify(4, 0, p)
    assert e.value.code == capi.SRH_E_INVALID
    with pytest.raises(capi.StereoHipError) as e:
        hip_ctx.depth_unrectify(2, 2, p)
    assert e.value.code == capi.SRH_E_INVALID


def test_plane(hip_ctx, small):
    """A slanted plane z = 20 + 0.5 x + 0.4 y through the rectified map and back.  The value a destination pixel gets is the
    plane's rectified depth at the CENTRE of the rectified pixel it read, carried along the destination pixel's own ray.
    In rectified pixel coordinates the plane's destination-camera depth is a ratio of two affine functions (extremes over a
    pixel at its corners), and the ratio of the two cameras' z along a ray is affine with a relative slope per pixel of at most
    sin(verging angle)/f = 0.05/61; the plane's own relative slope per pixel, 0.4/61 and more, is eight times that, so the
    value stays between the corner depths."""
    src, cams, p, rect = _rectified_small(hip_ctx, small)
    rw, rh, w, h = 67, 35, 61, 47
    s = p.image_scale
    n, d = np.array([-0.5, -0.4, 1.0]), 20.0

    def on_plane(cam, px, py):
        c, dirs = R.unproject(cam, px, py)
        tau = (d - n @ c) / (dirs @ n)
        assert (tau > 0).all()
        return c + dirs * tau[..., None]

    yy, xx = np.mgrid[0:rh, 0:rw]
    dr = R.local_z(rect[0], on_plane(rect[0], (xx + 0.5) / s, (yy + 0.5) / s))
    assert dr.min() > 5 and dr.max() / dr.min() > 1.5
    hip_ctx.upload_depth(2, dr)
    idx = hip_ctx.depth_unrectify(2, 0, p, want_index=True)
    got = hip_ctx.download_depth(0)
    hit = idx >= 0
    assert np.array_equal(np.isfinite(got), hit) and hit.sum() > 500
    xr, yr = idx[hit] % rw, idx[hit] // rw
    corners = np.stack([R.local_z(cams[0], on_plane(rect[0], (xr + dx) / s, (yr + dy) / s)) for dx in (0, 1) for dy in (0, 1)])
    lo, hi = corners.min(axis=0), corners.max(axis=0)
    assert ((got[hit] >= lo - TOL) & (got[hit] <= hi + TOL)).all()
    assert ((hi - lo) < 0.05 * lo).all()                         # (a pixel's corners are close: the band is a tight one)


def test_host_class(tmp_path, bunny):
    """tests/host_rectify_test.cpp: TwoViewStereo::setRectify on the example project's pair"""
    case, cams, p = bunny
    subprocess.check_call(["make", "-C", HA.HOST], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "host_rectify_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + HA.HOST,
                           os.path.join(ROOT, "tests", "host_rectify_test.cpp"), os.path.join(HA.HOST, "libstereo_recon_host.a"),
                           "-L" + HA.LIBDIR, "-lstereo_recon_hip", "-Wl,-rpath," + HA.LIBDIR, "-o", exe])
    h, w = case["views"][0][0].shape[:2]
    small_params = dict(case["params"], num_depth_levels=32)     # (three whole runs of the pair: a coarser sweep keeps them short)
    small_case = dict(case, params=small_params)
    inp = str(tmp_path / "in.bin")
    HA._write_input(inp, small_case, True)
    maps = {}
    for mode in ("off", "never", "on"):
        outp = str(tmp_path / ("out_%s.bin" % mode))
        subprocess.check_call([exe, mode, inp, outp])
        maps[mode], _ = HA._read_output(outp, 2, w, h)
    for s in (0, 1):                                             # setRectify(false): the maps of an object that never heard of it
        assert np.array_equal(maps["off"][s].view(np.uint64), maps["never"][s].view(np.uint64))
    left = maps["on"][0]
    fin = np.isfinite(left)
    assert left.shape == (h, w) and fin.sum() > 1000 and 38 < np.median(left[fin]) < 48
    assert np.isnan(left[case["views"][0][1] != 1]).all()
