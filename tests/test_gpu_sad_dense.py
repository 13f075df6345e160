"""The SAD matching cost on the row-aligned dense plan (option "sad_dense", twoview_strip_sad_kernel in srh_sad_strip.hip)
against the CPU restatement of TwoViewStereo::cost_sad and its WTA pass (tests/sad_restatement.cpp), against the row-run
path of the same context (sad_dense = 0) and, cost by cost, against the device's own pair costs.

Every map is compared bit for bit, NaN and inf positions included.  A test that claims the dense plan asserts
used_dense_path and used_strip_kernel after each pass: a silent fall-back cannot pass for the kernel.  The cost rows
equal srh_twoview_pair_costs bit for bit (the same windows, the same operations in the same order) and the CPU
restatement within 8 units in the last place (device exp against libm exp in the windows; tests/test_gpu_sad.py)."""
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
from stereoreconstruction_amd import capi, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "bunny_pair.npz")
HOST = os.path.join(ROOT, "stereoreconstruction_amd", "host")
LIBDIR = os.path.join(ROOT, "stereoreconstruction_amd")

DEFAULTS = dict(cost=capi.COST_NCC, sad_dense=0, list_rows=1, force_generic=0, force_dense=0, filter_invalid=0,
                tv_overlap=1, band_budget_mb=32768)

# (case, overrides) of tests/test_gpu_strip.py: image widths that are not a tile multiple, ranges that touch both image
# borders, masks (select-form candidates), radius 2, strips shorter and longer than an item
STRIP_CASES = [
    ("geodesic_rect", dict()),
    ("adaptive_rect", dict()),
    ("geodesic_masks", dict()),
    ("adaptive_masks", dict(w=97, h=53, D=24)),
    ("geodesic_r2", dict()),
    ("geodesic_rect", dict(w=200, h=70, D=48)),
    ("adaptive_rect", dict(w=161, h=37, D=130)),
    ("geodesic_scaled", dict()),
]


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


def _assert_same(got, want, tag):
    assert S.same_bits(got, want), "%s: %s" % (tag, S.diff_report(got, want))


def _assert_costs(got, want, tag, ulps=8):
    """the same special values in the same places, finite costs within `ulps` units in the last place"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(np.isnan(got), np.isnan(want)), tag
    assert np.array_equal(got[~fin], want[~fin]) or np.isnan(want[~fin]).all(), tag
    assert np.array_equal(got == 1000.0, want == 1000.0), tag + ": bad_ret positions"
    bad = np.abs(got[fin] - want[fin]) > ulps * np.spacing(np.abs(want[fin]))
    print("%s: %d costs, %d finite, largest difference %.3g ulp" % (
        tag, want.size, fin.sum(), (np.abs(got[fin] - want[fin]) / np.spacing(np.abs(want[fin]))).max() if fin.any() else 0.0))
    assert not bad.any(), "%s: %d of %d beyond %d ulp" % (tag, bad.sum(), fin.sum(), ulps)


def _case(name, **over):
    case = cases.get_twoview(name, **over)
    imgs, ocams, op = cases.oracle_inputs(case)
    cams, p = cases.hip_inputs(case)
    return case, imgs, ocams, op, cams, p


def _restated_maps(imgs, ocams, op):
    return [S.twoview_wta_sad(imgs[r], imgs[o], ocams[r], ocams[o], op) for r, o in ((0, 1), (1, 0))]


def _passes(ctx, p, dense):
    """both directions -> [(map, stats)]; on the dense plan every pass must have run the strip kernel"""
    out = []
    for ref, oth in ((0, 1), (1, 0)):
        ctx.twoview_wta(ref, oth, p)
        st = ctx.stats()
        if dense:
            assert st["used_dense_path"] and st["used_strip_kernel"], "direction %d>%d fell back: %s" % (ref, oth, st)
        else:
            assert not st["used_dense_path"], st
        out.append((ctx.download_depth(ref), st))
    return out


# ---------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("name,over", STRIP_CASES)
def test_shapes_against_restatement_and_row_runs(hip_ctx, name, over):
    case, imgs, ocams, op, cams, p = _case(name, **over)
    cases.upload_case(hip_ctx, case, cams)
    want = _restated_maps(imgs, ocams, op)
    with _options(hip_ctx, cost=capi.COST_SAD, sad_dense=1):
        got = _passes(hip_ctx, p, True)
    with _options(hip_ctx, cost=capi.COST_SAD, sad_dense=0):
        rows = _passes(hip_ctx, p, False)
    for d in range(2):
        tag = "%s %s direction %d" % (name, over, d)
        _assert_same(got[d][0], want[d], tag + " against the restatement")
        _assert_same(got[d][0], rows[d][0], tag + " against the row runs")
        assert got[d][1]["n_eval"] == rows[d][1]["n_eval"], tag
        assert np.isfinite(got[d][0]).mean() > 0.3, tag


# ---------------------------------------------------------------- 2. bands and row ranges
def test_row_ranges_and_small_budget(hip_ctx):
    case, imgs, ocams, op, cams, p = _case("geodesic_masks", w=96, h=64, D=20)
    cases.upload_case(hip_ctx, case, cams)
    with _options(hip_ctx, cost=capi.COST_SAD, sad_dense=1):
        hip_ctx.twoview_wta(0, 1, p)
        st = hip_ctx.stats()
        assert st["used_dense_path"] and st["used_strip_kernel"]
        full = hip_ctx.download_depth(0)
        _assert_same(full, S.twoview_wta_sad(imgs[0], imgs[1], ocams[0], ocams[1], op), "one band")
        hip_ctx.upload_depth(0, np.full(full.shape, np.nan))
        for y0, y1 in ((0, 7), (7, 30), (30, 64)):
            hip_ctx.twoview_wta(0, 1, p, y0, y1)
            st = hip_ctx.stats()
            assert st["used_dense_path"] and st["used_strip_kernel"]
        _assert_same(hip_ctx.download_depth(0), full, "row ranges")
        with _options(hip_ctx, band_budget_mb=1):
            hip_ctx.upload_depth(0, np.full(full.shape, np.nan))
            hip_ctx.twoview_wta(0, 1, p)
            st = hip_ctx.stats()
            assert st["used_dense_path"] and st["used_strip_kernel"]
            _assert_same(hip_ctx.download_depth(0), full, "band budget of 1 MB")


# ---------------------------------------------------------------- 3. cost rows
@pytest.mark.parametrize("name", ["geodesic_masks", "adaptive_rect", "geodesic_r2"])
def test_cost_rows_value_by_value(hip_ctx, name):
    case, imgs, ocams, op, cams, p = _case(name)
    cases.upload_case(hip_ctx, case, cams)
    h, w = case["views"][0][0].shape[:2]
    never = np.uint64(0xFFFFFFFFFFFFFFFF)
    for ref, oth in ((0, 1), (1, 0)):
        with _options(hip_ctx, cost=capi.COST_SAD, sad_dense=1):
            cost, rng, used_strip = hip_ctx.twoview_cost_rows(ref, oth, p, 0, h, 0)
        assert used_strip and cost.shape[:2] == (h, w)
        cstride = cost.shape[2]
        lo, hi = rng[..., 0].astype(np.int64), rng[..., 1].astype(np.int64)
        live = hi >= lo
        assert live.any() and (hi - lo + 1)[live].max() <= cstride
        k = np.arange(cstride)[None, None, :]
        inside = live[..., None] & (k <= (hi - lo)[..., None])
        bits = cost.view(np.uint64)
        assert not (bits[inside] == never).any(), "%s %d>%d: a column of [lo, hi] was never written" % (name, ref, oth)
        assert (bits[~inside] == never).all(), "%s %d>%d: an entry beyond hi was written" % (name, ref, oth)
        yy, xx, kk = np.nonzero(inside)
        xy = np.stack([xx, yy, lo[yy, xx] + kk, yy], 1).astype(np.int32)
        got = cost[yy, xx, kk]
        dev = hip_ctx.twoview_pair_costs(ref, oth, p, xy, capi.COST_SAD)
        _assert_same(got, dev, "%s %d>%d cost rows against the device's pair costs" % (name, ref, oth))
        want = S.pair_costs_sad(imgs[ref], imgs[oth], op, xy)
        _assert_costs(got, want, "%s %d>%d cost rows against the restatement" % (name, ref, oth))
    with _options(hip_ctx, cost=capi.COST_SAD, sad_dense=1):
        for form in (3, 5, 1, 2):
            with pytest.raises(capi.StereoHipError):
                hip_ctx.twoview_cost_rows(0, 1, p, 0, 4, form)
    with _options(hip_ctx, cost=capi.COST_SAD, sad_dense=0):
        with pytest.raises(capi.StereoHipError):
            hip_ctx.twoview_cost_rows(0, 1, p, 0, 4, 0)


# ---------------------------------------------------------------- 4. fall-backs
@pytest.mark.parametrize("name,over,extra", [
    ("adaptive_verged", dict(), dict()),
    ("geodesic_distorted", dict(), dict()),
    ("adaptive_rect", dict(w=400, h=24, D=330), dict()),                      # cstride + 32 > 320: wider than the chunk
    ("adaptive_verged", dict(w=72, h=44, D=20, radius=2), dict(force_dense=1)),  # proposed, refuted by the scan, redone
    ("geodesic_rect", dict(), dict(force_generic=1)),
], ids=["verged", "distorted", "wider_than_the_chunk", "force_dense_refuted", "force_generic"])
def test_fall_backs(hip_ctx, name, over, extra):
    case, imgs, ocams, op, cams, p = _case(name, **over)
    cases.upload_case(hip_ctx, case, cams)
    want = _restated_maps(imgs, ocams, op)
    with _options(hip_ctx, cost=capi.COST_SAD, sad_dense=1, **extra):
        got = _passes(hip_ctx, p, False)
        if name == "adaptive_rect":
            with pytest.raises(capi.StereoHipError):
                hip_ctx.twoview_cost_rows(0, 1, p, 0, 4, 0)
    for d in range(2):
        _assert_same(got[d][0], want[d], "%s %s direction %d" % (name, extra, d))


# ---------------------------------------------------------------- 5. whole pair
def _check_compute(ctx, case, imgs, ocams, op, p, tag, dense, filter_flags=0, **opts):
    dl, dr = _restated_maps(imgs, ocams, op)
    dl, dr = O.twoview_cross_check(ocams[0], ocams[1], op, dl, dr)
    if filter_flags:
        dl = F.filter_map(case["views"][0][0], case["views"][0][1], dl, F.oparams(p), filter_flags)
        dr = F.filter_map(case["views"][1][0], case["views"][1][1], dr, F.oparams(p), filter_flags)
    with _options(ctx, cost=capi.COST_SAD, sad_dense=1, filter_invalid=filter_flags, **opts):
        gl, gr = ctx.twoview_compute(0, 1, p)
        st = ctx.stats()
    assert bool(st["used_dense_path"]) == dense and bool(st["used_strip_kernel"]) == dense, (tag, st)
    _assert_same(gl, dl, tag + " left")
    _assert_same(gr, dr, tag + " right")
    return gl, gr


def _load_bunny():
    g = np.load(GOLD)
    views = []
    for tag in ("left", "right"):
        views.append((g[tag + "_rgba"], g[tag + "_mask"], (g[tag + "_K"], g[tag + "_R"], g[tag + "_t"]),
                      g[tag + "_dist"], None))
    params = dict(min_depth=30.0, max_depth=80.0, num_depth_levels=100, image_scale=float(g["scale"][0]),
                  window_radius=5, weight_kind=1)
    return dict(name="bunny", kind="twoview", views=views, params=params)


@pytest.mark.parametrize("which", ["geodesic_rect", "bunny"])
def test_compute_with_cross_check(hip_ctx, which):
    if which == "bunny":
        case = _load_bunny()
        imgs, ocams, op = cases.oracle_inputs(case)
        cams, p = cases.hip_inputs(case)
    else:
        case, imgs, ocams, op, cams, p = _case(which)
    cases.upload_case(hip_ctx, case, cams)
    dense = which != "bunny"                       # (the bunny pair is not row-aligned: the candidate lists)
    for ov in (1, 0):
        gl, gr = _check_compute(hip_ctx, case, imgs, ocams, op, p, "%s tv_overlap %d" % (which, ov), dense, tv_overlap=ov)
        assert np.isfinite(gl).sum() > 0 and np.isinf(gl).sum() + np.isnan(gl).sum() > 0
    _check_compute(hip_ctx, case, imgs, ocams, op, p, which + " filtered", dense, capi.FILTER_GAPS | capi.FILTER_MEDIAN)


# ---------------------------------------------------------------- 6. switching
def test_switching_on_one_context_and_reupload(hip_ctx):
    case, imgs, ocams, op, cams, p = _case("geodesic_rect")
    cases.upload_case(hip_ctx, case, cams)
    ncc1 = hip_ctx.twoview_compute(0, 1, p)
    with _options(hip_ctx, cost=capi.COST_SAD):
        sad_rows = hip_ctx.twoview_compute(0, 1, p)
        assert not hip_ctx.stats()["used_dense_path"]
    with _options(hip_ctx, cost=capi.COST_SAD, sad_dense=1):
        sad_dense = hip_ctx.twoview_compute(0, 1, p)
        st = hip_ctx.stats()
        assert st["used_dense_path"] and st["used_strip_kernel"]
    ncc2 = hip_ctx.twoview_compute(0, 1, p)
    for k in range(2):
        _assert_same(ncc2[k], ncc1[k], "ncc again %d" % k)
        _assert_same(sad_dense[k], sad_rows[k], "sad dense against row runs %d" % k)
        assert not S.same_bits(sad_dense[k], ncc1[k])
    # other views into the same slots: the cached planes of the old ones must not survive
    case, imgs, ocams, op, cams, p = _case("geodesic_masks")
    cases.upload_case(hip_ctx, case, cams)
    want = _restated_maps(imgs, ocams, op)
    with _options(hip_ctx, cost=capi.COST_SAD, sad_dense=1):
        got = _passes(hip_ctx, p, True)
    for d in range(2):
        _assert_same(got[d][0], want[d], "after the re-upload, direction %d" % d)
        assert not S.same_bits(got[d][0], sad_dense[d])


# ---------------------------------------------------------------- 7. full size
def _rows(H, R=5):
    """8 stratified rows: the first and last, the rows either side of where windows stop crossing the border, interior"""
    rows = [0, R - 1, R, H // 3, H // 2 + 7, H - R - 1, H - R, H - 1]
    assert len(set(rows)) == 8
    return rows


def _c3():
    W, H, D = 1920, 1080, 256
    L, R, ml, mr, _ = synthetic.rectified_pair(W, H, D, 0x5EED0003)
    cams = synthetic.rectified_cameras(W, H)
    zmin, zmax = synthetic.rectified_depth_range(W, D)
    kw = dict(min_depth=zmin, max_depth=zmax, num_depth_levels=D, weight_kind=capi.WEIGHT_GEODESIC)
    return W, H, L, R, ml, mr, cams, kw


def _upload_c3(ctx, L, R, ml, mr, cams):
    (Kl, Rl, tl), (Kr, Rr, tr) = cams
    ctx.upload_view(0, L, ml, capi.camera_from_krt(Kl, Rl, tl, None, None, 0.0, 1.0))
    ctx.upload_view(1, R, mr, capi.camera_from_krt(Kr, Rr, tr, None, None, 0.0, 1.0))


def test_full_size_dense_against_row_runs_and_restated_rows(hip_ctx):
    W, H, L, R, ml, mr, cams, kw = _c3()
    (Kl, Rl, tl), (Kr, Rr, tr) = cams
    _upload_c3(hip_ctx, L, R, ml, mr, cams)
    p = capi.params_twoview(**kw)
    op = O.params_twoview(**kw)
    oc = [O.camera_set(Kl, Rl, tl, None, None, 0.0, 1.0), O.camera_set(Kr, Rr, tr, None, None, 0.0, 1.0)]
    oi = [O.OImage(L, ml), O.OImage(R, mr)]
    with _options(hip_ctx, cost=capi.COST_SAD, sad_dense=1):
        got = _passes(hip_ctx, p, True)
    with _options(hip_ctx, cost=capi.COST_SAD, sad_dense=0):
        rows_maps = _passes(hip_ctx, p, False)
    rows = _rows(H)
    for d, (ref, oth) in enumerate(((0, 1), (1, 0))):
        _assert_same(got[d][0], rows_maps[d][0], "C3 %d>%d dense against row runs" % (ref, oth))
        with ThreadPoolExecutor(max_workers=8) as ex:
            want = list(ex.map(lambda y: S.twoview_wta_sad(oi[ref], oi[oth], oc[ref], oc[oth], op, y, y + 1)[y], rows))
        for y, wrow in zip(rows, want):
            _assert_same(got[d][0][y], wrow, "C3 %d>%d row %d" % (ref, oth, y))
        assert np.isfinite(got[d][0]).mean() > 0.2


def test_full_size_ragged_mask_dense_against_row_runs(hip_ctx):
    """60 % of the other view's mask cleared in ragged runs: most candidate windows hold a masked tap, the select form
    carries the load"""
    W, H, L, R, ml, mr, cams, kw = _c3()
    rng = np.random.default_rng(0x5AD0DE45)
    mr = np.ones((H, W), np.uint8) if mr is None else np.array(mr, np.uint8)
    keep = np.ones((H, W), bool)
    for y in range(H):
        x = 0
        while x < W:
            run = int(rng.integers(1, 40))
            if rng.random() < 0.6:
                keep[y, x:x + run] = False
            x += run
    mr = (mr.astype(bool) & keep).astype(np.uint8)
    assert 0.3 < mr.mean() < 0.5
    _upload_c3(hip_ctx, L, R, ml, mr, cams)
    p = capi.params_twoview(**kw)
    with _options(hip_ctx, cost=capi.COST_SAD, sad_dense=1):
        got = _passes(hip_ctx, p, True)
    with _options(hip_ctx, cost=capi.COST_SAD, sad_dense=0):
        rows_maps = _passes(hip_ctx, p, False)
    for d in range(2):
        _assert_same(got[d][0], rows_maps[d][0], "C3 ragged mask, direction %d, dense against row runs" % d)
    assert np.isfinite(got[0][0]).sum() > 0


# ---------------------------------------------------------------- 8. the host class's setter
def test_host_class_setter(hip_ctx, tmp_path):
    import test_gpu_host_api as HA
    subprocess.check_call(["make", "-C", HA.HOST], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "host_sad_dense_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + HA.HOST,
                           os.path.join(ROOT, "tests", "host_sad_dense_test.cpp"),
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
    for on in (0, 1):
        outp = str(tmp_path / ("out%d.bin" % on))
        subprocess.check_call([exe, inp, outp, str(on)])
        (gl, gr), steps = HA._read_output(outp, 2, w, h)
        assert steps == [1, 3, 5, 8]
        _assert_same(gl, want[0], "host left, setSadDense(%d)" % on)
        _assert_same(gr, want[1], "host right, setSadDense(%d)" % on)
