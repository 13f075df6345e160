"""The by-products of the TwoView WTA scan (option "wta_outputs", srh_view_wta_outputs*): winner, runner-up and their
costs per reference pixel, against the CPU oracle's diagnostics, across every plan of the library, against
srh_twoview_pair_costs, against the depth map of the same pass, over row ranges and bands, and through the host class."""
import contextlib
import ctypes as C
import math
import struct
import subprocess

import numpy as np
import pytest

import cases
import oracle_ffi as O
import sad_ref as S
import test_gpu_host_api as HA
from stereoreconstruction_amd import capi, synthetic
from test_gpu_arith_modes import _adversarial_pair
from test_wta_outputs_host import build_host_program

pytestmark = pytest.mark.gpu

DEFAULTS = dict(wta_outputs=0, arith=capi.ARITH_DEFAULT, strip=1, tscan=1, fused=0, force_generic=0, list_rows=1,
                tv_overlap=1, cost=capi.COST_NCC, sad_dense=0, band_budget_mb=32768)
PLANES = ("win_xy", "runner_xy", "min_cost", "second_cost")


@contextlib.contextmanager
def _options(ctx, **opts):
    """set options on the shared context, and put the defaults back whatever happens"""
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k in opts:
            ctx.set_option(k, DEFAULTS[k])
        ctx.set_option("wta_outputs", 0)


def _setup(ctx, name, **over):
    case = cases.get_twoview(name, **over)
    cams, p = cases.hip_inputs(case)
    cases.upload_case(ctx, case, cams)
    return case, p


def _pass(ctx, ref, oth, p, y0=0, y1=0):
    """one WTA pass -> (depth map, planes, stats)"""
    ctx.twoview_wta(ref, oth, p, y0, y1)
    return ctx.download_depth(ref), ctx.wta_outputs(ref), ctx.stats()


def _same_planes(got, want, tag, rows=None):
    for k in PLANES:
        if k not in want and k not in got:
            continue
        a, b = got[k], want[k]
        if rows is not None:
            a, b = a[rows[0]:rows[1]], b[rows[0]:rows[1]]
        if a.dtype == np.float64:
            a, b = np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)
        assert np.array_equal(a, b), "%s: %s differs at %d places, first %s" % (tag, k, (a != b).sum(), np.argwhere(a != b)[:3].tolist())


def _yardstick(ctx, p):
    """the walk kernel in the reference's arithmetic, both directions"""
    with _options(ctx, wta_outputs=3, force_generic=2, arith=0):
        out = [_pass(ctx, a, b, p) for a, b in ((0, 1), (1, 0))]
    for d, o, st in out:
        assert not st["used_dense_path"]
    return out


# ---------------------------------------------------------------------------------------------- 1. against the oracle
ORACLE_CASES = ["geodesic_rect", "adaptive_masks", "geodesic_r2", "geodesic_verged_dist_masks", "adaptive_refractive"]


def _decision_gap(imgs, ocams, op, ref, oth, x, y):
    """replay of the oracle's scan of one pixel: how close its closest decision is to flipping"""
    curve = O.epipolar_curve(ocams[ref], ocams[oth], imgs[oth], op, False, x, y)
    wts = np.ascontiguousarray(O.weights(imgs[ref], x, y, op), dtype=np.float64)
    min_cost, second, win, gap = math.inf, math.inf, None, math.inf
    for cx, cy in curve:
        cx, cy = int(cx), int(cy)
        cost = O.lib().sro_twoview_cost_ncc(C.byref(imgs[ref].c), C.byref(imgs[oth].c), O.dptr(wts), C.byref(op), x, y, cx, cy)
        if math.isfinite(min_cost) and (cx, cy) != win:
            gap = min(gap, abs(cost + op.wta_margin - min_cost))
        if cost + op.wta_margin < min_cost:
            second, min_cost, win = min_cost, cost, (cx, cy)
    if math.isfinite(min_cost) and math.isfinite(second):
        gap = min(gap, abs(min_cost - op.second_best_factor * second))
    return gap


def _close(got, want):
    """+INF in the same places, finite costs within 1e-9 relative (device exp against libm's, tests/test_gpu_sad.py)"""
    fin = np.isfinite(want)
    ok = np.isfinite(got) == fin
    ok &= np.where(fin, np.abs(np.where(fin, got, 0) - np.where(fin, want, 0)) <= 1e-9 * np.maximum(1.0, np.abs(np.where(fin, want, 0))),
                   got == want)
    return ok


def compare_planes_with_the_oracle(got, diag, white, imgs, ocams, op, ref, oth, name):
    """The decision-gap rule: winners equal and both costs within 1e-9 relative of the oracle's diagnostics, except at pixels
    whose closest decision the oracle's own replay puts within 1e-7 of flipping -- at most 1 % of the WHITE pixels; nothing
    outside the mask.  -> the number of pixels excused (tests/test_gpu_radii_twoview.py applies it at other radii)"""
    agree = (got["win_xy"] == diag["win_xy"]).all(axis=2) & _close(got["min_cost"], diag["min_cost"]) & \
        _close(got["second_cost"], diag["second_cost"])
    bad = np.argwhere(~agree)
    print("%s %d>%d: %d of %d WHITE pixels disagree with the oracle" % (name, ref, oth, len(bad), white.sum()))
    for y, x in bad:
        gap = _decision_gap(imgs, ocams, op, ref, oth, int(x), int(y))
        print("  (%d,%d): win %s / %s, min %r / %r, second %r / %r, decision gap %.3g" % (
            x, y, got["win_xy"][y, x], diag["win_xy"][y, x], got["min_cost"][y, x], diag["min_cost"][y, x],
            got["second_cost"][y, x], diag["second_cost"][y, x], gap))
        assert gap <= 1e-7, "%s %d>%d pixel (%d,%d): disagrees with the oracle, no decision within 1e-7 of flipping (gap %g)" % (name, ref, oth, x, y, gap)
    assert len(bad) <= 0.01 * white.sum()
    # outside the mask: nothing
    assert (got["win_xy"][~white] == -1).all() and (got["runner_xy"][~white] == -1).all()
    assert np.isposinf(got["min_cost"][~white]).all() and np.isposinf(got["second_cost"][~white]).all()
    return len(bad)


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_planes_against_the_oracle(hip_ctx, name):
    case, p = _setup(hip_ctx, name)
    imgs, ocams, op = cases.oracle_inputs(case)
    for ref, oth in ((0, 1), (1, 0)):
        _, diag = O.twoview_wta(imgs[ref], imgs[oth], ocams[ref], ocams[oth], op, want_diag=True)
        with _options(hip_ctx, wta_outputs=3):
            _, got, _ = _pass(hip_ctx, ref, oth, p)
        white = case["views"][ref][1] == 1
        compare_planes_with_the_oracle(got, diag, white, imgs, ocams, op, ref, oth, name)
        # the awkward classes occur: no candidate at all, a single improvement (no runner-up)
        none = white & (got["win_xy"][..., 0] < 0)
        single = (got["win_xy"][..., 0] >= 0) & (got["runner_xy"][..., 0] < 0)
        print("  no candidate: %d pixels, single improvement: %d pixels" % (none.sum(), single.sum()))
        assert none.sum() > 0 and single.sum() > 0
        assert np.isposinf(got["min_cost"][none]).all() and np.isposinf(got["second_cost"][single]).all()
        assert np.isfinite(got["min_cost"][got["win_xy"][..., 0] >= 0]).all()
        assert np.isfinite(got["second_cost"][got["runner_xy"][..., 0] >= 0]).all()


# ---------------------------------------------------------------------------------------------- 2. every path, same bits
def _dense(st):
    return st["used_dense_path"]


RECT_PATHS = [
    ("defaults", dict(), lambda st: _dense(st) and (st["scan_tiles_template"] > 0 or st["scan_tiles_walked"] > 0)),
    ("arith 0", dict(arith=0), lambda st: _dense(st) and st["n_certified"] == 0),
    ("strip 0", dict(strip=0), lambda st: _dense(st) and not st["used_strip_kernel"]),
    ("strip 4", dict(strip=4), lambda st: _dense(st) and st["used_strip_kernel"]),
    ("strip 8", dict(strip=8), lambda st: _dense(st) and st["used_strip_kernel"]),
    ("tscan 0", dict(tscan=0), lambda st: _dense(st) and st["scan_tiles_template"] == 0),
    ("fused", dict(fused=1), lambda st: st["used_fused_kernel"]),
    ("row-run lists", dict(force_generic=1, list_rows=1), lambda st: not _dense(st) and not st["used_fused_kernel"]),
    ("list order", dict(force_generic=1, list_rows=0), lambda st: not _dense(st) and not st["used_fused_kernel"]),
]
GENERAL_PATHS = [
    ("defaults", dict(), lambda st: not _dense(st)),
    ("list order", dict(list_rows=0), lambda st: not _dense(st)),
    ("arith 0", dict(arith=0), lambda st: not _dense(st)),
]


@pytest.mark.parametrize("name", ["geodesic_rect", "adaptive_rect", "geodesic_r2"])
def test_every_rectified_path_gives_the_walk_kernels_bits(hip_ctx, name):
    case, p = _setup(hip_ctx, name)
    want = _yardstick(hip_ctx, p)
    for tag, opts, ran in RECT_PATHS:
        with _options(hip_ctx, wta_outputs=3, **opts):
            for k, (ref, oth) in enumerate(((0, 1), (1, 0))):
                d, got, st = _pass(hip_ctx, ref, oth, p)
                assert ran(st), "%s %s: the intended path did not run: %s" % (name, tag, st)
                _same_planes(got, want[k][1], "%s %s %d>%d" % (name, tag, ref, oth))
                assert S.same_bits(d, want[k][0]), "%s %s: depth map" % (name, tag)
    for overlap in (1, 0):
        with _options(hip_ctx, wta_outputs=3, tv_overlap=overlap):
            hip_ctx.twoview_compute(0, 1, p)
            st = hip_ctx.stats()
            assert st["used_dense_path"]
            for k in range(2):
                assert hip_ctx.wta_outputs_state(k) == (3, 1 - k)
                _same_planes(hip_ctx.wta_outputs(k), want[k][1], "%s compute tv_overlap=%d slot %d" % (name, overlap, k))


@pytest.mark.parametrize("name", ["geodesic_verged_dist_masks", "adaptive_refractive"])
def test_every_general_path_gives_the_walk_kernels_bits(hip_ctx, name):
    case, p = _setup(hip_ctx, name)
    want = _yardstick(hip_ctx, p)
    for tag, opts, ran in GENERAL_PATHS:
        with _options(hip_ctx, wta_outputs=3, **opts):
            for k, (ref, oth) in enumerate(((0, 1), (1, 0))):
                d, got, st = _pass(hip_ctx, ref, oth, p)
                assert ran(st), "%s %s: the intended path did not run: %s" % (name, tag, st)
                _same_planes(got, want[k][1], "%s %s %d>%d" % (name, tag, ref, oth))
                assert S.same_bits(d, want[k][0]), "%s %s: depth map" % (name, tag)


# ---------------------------------------------------------------------------------------------- 3. flagged pixels
@pytest.mark.parametrize("strip", [8, 0], ids=["strip", "per-tile"])
def test_flagged_pixels_keep_the_exact_scans_planes(hip_ctx, strip):
    W, H, D = 192, 96, 40
    L, R, ml, mr = _adversarial_pair("periodic", W, H, D)
    (Kl, Rl, tl), (Kr, Rr, tr) = synthetic.rectified_cameras(W, H)
    zmin, zmax = synthetic.rectified_depth_range(W, D)
    hip_ctx.upload_view(0, L, ml, capi.camera_from_krt(Kl, Rl, tl))
    hip_ctx.upload_view(1, R, mr, capi.camera_from_krt(Kr, Rr, tr))
    p = capi.params_twoview(min_depth=zmin, max_depth=zmax, num_depth_levels=D, weight_kind=capi.WEIGHT_GEODESIC)
    flagged = 0
    for ref, oth in ((0, 1), (1, 0)):
        with _options(hip_ctx, wta_outputs=3, strip=strip, arith=0):
            d0, exact, st0 = _pass(hip_ctx, ref, oth, p)
        with _options(hip_ctx, wta_outputs=3, strip=strip, arith=3):
            d3, cert, st3 = _pass(hip_ctx, ref, oth, p)
        assert st0["used_dense_path"] and st3["used_dense_path"] and st3["n_certified"] > 0
        assert bool(st3["used_strip_kernel"]) == (strip != 0)
        flagged += st3["n_flagged"]
        _same_planes(cert, exact, "periodic strip=%d %d>%d" % (strip, ref, oth))
        assert S.same_bits(d3, d0)
    print("periodic, strip=%d: %d pixels flagged and redone" % (strip, flagged))
    assert flagged > 0, "an image made of exact ties must trip the bound somewhere"


# ---------------------------------------------------------------------------------------------- 4. the costs are pair costs
def _assert_pair_costs(ctx, ref, oth, p, planes, kind, tag):
    """-> the (x, y, win) and (x, y, runner) pairs; min_cost / second_cost are srh_twoview_pair_costs of them, bit for bit"""
    out = []
    for xyk, ck in (("win_xy", "min_cost"), ("runner_xy", "second_cost")):
        have = planes[xyk][..., 0] >= 0
        ys, xs = np.nonzero(have)
        xy = np.stack([xs, ys, planes[xyk][ys, xs, 0], planes[xyk][ys, xs, 1]], 1).astype(np.int32)
        assert len(xy) > 0
        want = ctx.twoview_pair_costs(ref, oth, p, xy, kind)
        got = planes[ck][ys, xs]
        assert S.same_bits(got, want), "%s %s: %s" % (tag, ck, S.diff_report(got, want))
        assert np.isposinf(planes[ck][~have]).all(), tag
        out.append((xy, got))
    return out


@pytest.mark.parametrize("arith", [3, 0, 1, 2])
@pytest.mark.parametrize("name", ["geodesic_rect", "adaptive_masks"])
def test_costs_are_ncc_pair_costs_under_every_arithmetic(hip_ctx, name, arith):
    case, p = _setup(hip_ctx, name)
    for ref, oth in ((0, 1), (1, 0)):
        with _options(hip_ctx, wta_outputs=3, arith=arith):
            _, planes, st = _pass(hip_ctx, ref, oth, p)
        assert st["used_dense_path"]
        _assert_pair_costs(hip_ctx, ref, oth, p, planes, capi.COST_NCC, "%s arith %d %d>%d" % (name, arith, ref, oth))


@pytest.mark.parametrize("sad_dense", [0, 1])
@pytest.mark.parametrize("name", ["geodesic_rect", "adaptive_masks", "geodesic_verged_dist_masks"])
def test_costs_are_sad_pair_costs(hip_ctx, name, sad_dense):
    case, p = _setup(hip_ctx, name)
    imgs, ocams, op = cases.oracle_inputs(case)
    for ref, oth in ((0, 1), (1, 0)):
        with _options(hip_ctx, wta_outputs=3, cost=capi.COST_SAD, sad_dense=sad_dense):
            _, planes, st = _pass(hip_ctx, ref, oth, p)
        if name != "geodesic_verged_dist_masks":
            assert bool(st["used_dense_path"]) == bool(sad_dense), st
        tag = "%s sad_dense=%d %d>%d" % (name, sad_dense, ref, oth)
        for xy, got in _assert_pair_costs(hip_ctx, ref, oth, p, planes, capi.COST_SAD, tag):
            # ... and the CPU restatement's, within its 8 units in the last place (tests/test_gpu_sad.py)
            want = S.pair_costs_sad(imgs[ref], imgs[oth], op, xy)
            assert np.array_equal(got == op.bad_ret, want == op.bad_ret), tag
            assert (np.abs(got - want) <= 8 * np.spacing(np.abs(want))).all(), tag


# ---------------------------------------------------------------------------------------------- 5. the depth map of the same pass
@pytest.mark.parametrize("name", ["geodesic_rect", "adaptive_masks", "geodesic_verged_dist_masks", "adaptive_refractive"])
def test_planes_are_consistent_with_the_depth_map_of_the_pass(hip_ctx, name):
    case, p = _setup(hip_ctx, name)
    for ref, oth in ((0, 1), (1, 0)):
        with _options(hip_ctx, wta_outputs=3):
            depth, planes, _ = _pass(hip_ctx, ref, oth, p)
        none = planes["win_xy"][..., 0] < 0
        assert np.array_equal(none, (planes["win_xy"] == -1).all(axis=2))
        assert np.array_equal(np.isnan(depth), none)
        with np.errstate(invalid="ignore"):
            rejected = ~none & (planes["min_cost"] > p.second_best_factor * planes["second_cost"])
        assert np.array_equal(np.isposinf(depth), rejected)
        assert np.isfinite(depth[~none & ~rejected]).all()
        ys, xs = np.nonzero(~none)
        curves = hip_ctx.epipolar_curves(ref, oth, p, np.stack([xs, ys], 1).astype(np.int32))
        for x, y, curve in zip(xs, ys, curves):
            for k in ("win_xy", "runner_xy"):
                c = planes[k][y, x]
                assert c[0] < 0 or (curve == c).all(axis=1).any(), "%s %d>%d (%d,%d): %s %s is not on the pixel's curve" % (name, ref, oth, x, y, k, c)


# ---------------------------------------------------------------------------------------------- 6. rows and bands
@pytest.mark.parametrize("name,opts", [("geodesic_rect", dict()), ("geodesic_rect", dict(strip=8)), ("geodesic_verged_dist_masks", dict()),
                                       ("geodesic_verged_dist_masks", dict(list_rows=0)), ("adaptive_rect", dict(force_generic=2))])
def test_a_row_range_writes_its_rows_only(hip_ctx, name, opts):
    case, p = _setup(hip_ctx, name)
    with _options(hip_ctx, wta_outputs=3, **opts):
        _, full, _ = _pass(hip_ctx, 0, 1, p)
    cams, _ = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)                         # freshly uploaded views
    with _options(hip_ctx, wta_outputs=3, **opts):
        _, part, _ = _pass(hip_ctx, 0, 1, p, 7, 19)
    _same_planes(part, full, "%s rows [7,19)" % name, rows=(7, 19))
    for rows in ((0, 7), (19, None)):
        sl = slice(*rows)
        assert (part["win_xy"][sl] == -1).all() and (part["runner_xy"][sl] == -1).all()
        assert np.isposinf(part["min_cost"][sl]).all() and np.isposinf(part["second_cost"][sl]).all()


# (the verged case at radius 5 instead of its own 2: 1 MB, the smallest budget there is, holds all 40 rows of radius-2 windows)
@pytest.mark.parametrize("name,over,opts", [("geodesic_rect", dict(), dict()), ("geodesic_rect", dict(), dict(strip=8)),
                                            ("geodesic_verged_dist_masks", dict(radius=5), dict()),
                                            ("geodesic_verged_dist_masks", dict(radius=5), dict(list_rows=0)),
                                            ("adaptive_rect", dict(), dict(force_generic=2))])
def test_bands_give_the_bits_of_one_band(hip_ctx, name, over, opts):
    case, p = _setup(hip_ctx, name, **over)
    h, w = case["views"][0][0].shape[:2]
    taps = (2 * p.window_radius + 1) ** 2
    # a band holds at least its windows: at most this many rows fit 1 MB, so the pass takes at least 3 bands
    assert math.ceil(h / ((1 << 20) // (taps * 8 * w))) >= 3
    for ref, oth in ((0, 1), (1, 0)):
        with _options(hip_ctx, wta_outputs=3, **opts):
            d1, one, _ = _pass(hip_ctx, ref, oth, p)
        with _options(hip_ctx, wta_outputs=3, band_budget_mb=1, **opts):
            dn, many, _ = _pass(hip_ctx, ref, oth, p)
        _same_planes(many, one, "%s %s banded %d>%d" % (name, opts, ref, oth))
        assert S.same_bits(dn, d1)


# ---------------------------------------------------------------------------------------------- 7. state
def _invalid(fn, *a, **kw):
    with pytest.raises(capi.StereoHipError) as e:
        fn(*a, **kw)
    assert e.value.code == capi.SRH_E_INVALID, e.value
    return e.value


def test_option_values_and_getter_states(hip_ctx):
    case, p = _setup(hip_ctx, "geodesic_rect")
    cams, _ = cases.hip_inputs(case)
    E_INVALID = capi.SRH_E_INVALID
    for bad in (2, -1, 4, 7):
        _invalid(hip_ctx.set_option, "wta_outputs", bad)
    try:
        # before any pass
        hip_ctx.set_option("wta_outputs", 3)
        assert hip_ctx.wta_outputs_state(0) == (0, -1)
        assert _invalid(hip_ctx.wta_outputs, 0, True).code == E_INVALID
        assert _invalid(hip_ctx.wta_outputs_device, 0).code == E_INVALID
        hip_ctx.twoview_wta(0, 1, p)
        assert hip_ctx.wta_outputs_state(0) == (3, 1) and hip_ctx.wta_outputs_state(1) == (0, -1)
        dev = hip_ctx.wta_outputs_device(0)
        assert all(dev) and len(set(dev)) == 4
        full = hip_ctx.wta_outputs(0)
        d3 = hip_ctx.download_depth(0)
        # after a re-upload
        cases.upload_case(hip_ctx, case, cams)
        assert hip_ctx.wta_outputs_state(0) == (0, -1)
        assert _invalid(hip_ctx.wta_outputs, 0).code == E_INVALID
        # winners only: no cost planes, the same winners, the same depth bits
        hip_ctx.set_option("wta_outputs", 1)
        hip_ctx.twoview_wta(0, 1, p)
        assert hip_ctx.wta_outputs_state(0) == (1, 1)
        only = hip_ctx.wta_outputs(0)
        assert sorted(only) == ["runner_xy", "win_xy"]
        _same_planes(only, dict(win_xy=full["win_xy"], runner_xy=full["runner_xy"]), "winners only")
        assert _invalid(hip_ctx.wta_outputs, 0, True).code == E_INVALID
        assert _invalid(hip_ctx.wta_outputs_device, 0, True).code == E_INVALID
        assert all(hip_ctx.wta_outputs_device(0, False)[:2])
        d1 = hip_ctx.download_depth(0)
        # option off: the depth map's bits again, and the slot holds nothing
        hip_ctx.set_option("wta_outputs", 0)
        hip_ctx.twoview_wta(0, 1, p)
        assert hip_ctx.wta_outputs_state(0) == (0, -1)
        assert _invalid(hip_ctx.wta_outputs, 0).code == E_INVALID
        d0 = hip_ctx.download_depth(0)
        assert S.same_bits(d0, d1) and S.same_bits(d0, d3)
        # the MRF stage makes a depth map without a scan: the planes are stale
        hip_ctx.set_option("wta_outputs", 3)
        hip_ctx.twoview_wta(0, 1, p)
        assert hip_ctx.wta_outputs_state(0) == (3, 1)
        hip_ctx.twoview_mrf(0, 1, p)
        assert hip_ctx.wta_outputs_state(0) == (0, -1)
        assert _invalid(hip_ctx.wta_outputs, 0).code == E_INVALID
    finally:
        hip_ctx.set_option("wta_outputs", 0)


def test_compute_depth_maps_do_not_depend_on_the_option(hip_ctx):
    case, p = _setup(hip_ctx, "adaptive_masks")
    maps = {}
    for flags in (0, 1, 3):
        with _options(hip_ctx, wta_outputs=flags):
            maps[flags] = hip_ctx.twoview_compute(0, 1, p)
            assert hip_ctx.wta_outputs_state(0) == ((flags, 1) if flags else (0, -1))
    for flags in (1, 3):
        for k in range(2):
            assert S.same_bits(maps[flags][k], maps[0][k])


# ---------------------------------------------------------------------------------------------- 8. host class
def _read_host_output(path, w, h):
    raw = open(path, "rb").read()
    n = w * h
    off = 2 * n * 8
    counts = struct.unpack_from("<8i", raw, off)
    off += 32
    out = []
    for k, cnt in enumerate(counts):
        dt = np.int32 if k % 4 < 2 else np.float64
        out.append(np.frombuffer(raw, dt, cnt, off))
        off += cnt * np.dtype(dt).itemsize
    assert off == len(raw)
    return out


def test_host_class_accessors_equal_the_c_abi_download(hip_ctx, tmp_path):
    exe = build_host_program(tmp_path)
    case = cases.get_twoview("geodesic_masks", w=48, h=36)
    w, h = 48, 36
    inp = str(tmp_path / "in.bin")
    HA._write_input(inp, case, True)
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    with _options(hip_ctx, wta_outputs=3):
        hip_ctx.twoview_compute(0, 1, p)
        want = [hip_ctx.wta_outputs(k) for k in range(2)]
    for flags in (3, 1, 0):
        outp = str(tmp_path / ("out%d.bin" % flags))
        subprocess.check_call([exe, inp, outp, str(flags)])
        got = _read_host_output(outp, w, h)
        for side in range(2):
            for j, k in enumerate(PLANES):
                a = got[4 * side + j]
                if flags == 0 or (flags == 1 and j >= 2):
                    assert a.size == 0, (flags, side, k)
                    continue
                b = want[side][k].reshape(-1)
                assert a.size == b.size, (flags, side, k)
                if b.dtype == np.float64:
                    assert S.same_bits(a, b), (flags, side, k)
                else:
                    assert np.array_equal(a, b), (flags, side, k)
    # under the MRF stage no scan makes the maps: empty vectors
    outp = str(tmp_path / "out_mrf.bin")
    subprocess.check_call([exe, inp, outp, "3", "mrf"])
    assert all(a.size == 0 for a in _read_host_output(outp, w, h))
