"""The census matching cost on the row-aligned dense plan (option "census_dense", twoview_strip_census_kernel in
srh_census_strip.hip) against the CPU restatement of the cost and its WTA pass
(tests/census_restatement.cpp), against the candidate lists of the same context (census_dense = 0) and, cost by cost,
against the device's own pair costs.

Every map is compared bit for bit, NaN and inf positions included.  A test that claims the kernel asserts used_dense_path
and used_strip_kernel after each pass: a silent fall-back cannot pass for the kernel.  The cost rows equal
srh_twoview_pair_costs bit for bit (the same windows, the same operations in the same order) and the CPU restatement
within 8 units in the last place (device exp against libm exp in the windows; tests/test_gpu_census.py).

Tiny views: the kernel RUNS on every shape of small_shapes.TWOVIEW_SHAPES, the 1 x 1 view and the one-row and one-column
views included (their planes in the padded raster cover every staged piece); none declines to the lists."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

import cases
import census_ref as CR
import constants_cases as CC
import filter_ref as F
import oracle_ffi as O
import small_shapes as SS
from stereoreconstruction_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECTIONS = ((0, 1), (1, 0))

DEFAULTS = dict(cost=capi.COST_NCC, census_dense=0, sad_dense=0, list_rows=1, force_generic=0, force_dense=0, filter_invalid=0,
                tv_overlap=1, band_budget_mb=32768, wta_outputs=0, subpixel=0)

# (case, overrides) of tests/test_gpu_sad_dense.py: image widths that are not a tile multiple, ranges that touch both image
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
    assert CR.same_bits(got, want), "%s: %s" % (tag, CR.diff_report(got, want))


def _assert_costs(got, want, tag, bad_ret=1000.0, ulps=8):
    """the same special values in the same places, finite costs within `ulps` units in the last place"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(np.isnan(got), np.isnan(want)), tag
    assert np.array_equal(got[~fin], want[~fin]) or np.isnan(want[~fin]).all(), tag
    assert np.array_equal(got == bad_ret, want == bad_ret), tag + ": bad_ret positions"
    err = np.abs(got[fin] - want[fin]) / np.spacing(np.maximum(np.abs(want[fin]), np.finfo(np.float64).tiny))
    print("%s: %d costs, %d finite, largest difference %.3g ulp" % (tag, want.size, fin.sum(), err.max() if fin.any() else 0.0))
    assert not (err > ulps).any(), "%s: %d of %d beyond %d ulp" % (tag, (err > ulps).sum(), fin.sum(), ulps)


def _case(name, **over):
    case = cases.get_twoview(name, **over)
    imgs, ocams, op = cases.oracle_inputs(case)
    cams, p = cases.hip_inputs(case)
    return case, imgs, ocams, op, cams, p


def _restated_maps(imgs, ocams, op):
    return [CR.twoview_wta_census(imgs[r], imgs[o], ocams[r], ocams[o], op) for r, o in DIRECTIONS]


def _passes(ctx, p, dense):
    """both directions -> [(map, stats)]; on the dense plan every pass must have run the strip kernel"""
    out = []
    for ref, oth in DIRECTIONS:
        ctx.twoview_wta(ref, oth, p)
        st = ctx.stats()
        if dense:
            assert st["used_dense_path"] and st["used_strip_kernel"], "direction %d>%d fell back: %s" % (ref, oth, st)
        else:
            assert not st["used_dense_path"], st
        out.append((ctx.download_depth(ref), st))
    return out


def _dense_and_lists(ctx, p):
    with _options(ctx, cost=capi.COST_CENSUS, census_dense=1):
        got = _passes(ctx, p, True)
    with _options(ctx, cost=capi.COST_CENSUS, census_dense=0):
        lists = _passes(ctx, p, False)
    return got, lists


# ---------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("name,over", STRIP_CASES)
def test_shapes_against_restatement_and_lists(hip_ctx, name, over):
    case, imgs, ocams, op, cams, p = _case(name, **over)
    cases.upload_case(hip_ctx, case, cams)
    want = _restated_maps(imgs, ocams, op)
    got, lists = _dense_and_lists(hip_ctx, p)
    for d in range(2):
        tag = "%s %s direction %d" % (name, over, d)
        _assert_same(got[d][0], want[d], tag + " against the restatement")
        _assert_same(got[d][0], lists[d][0], tag + " against the lists")
        assert got[d][1]["n_eval"] == lists[d][1]["n_eval"], tag
        assert np.isfinite(got[d][0]).mean() > 0.3, tag


# ---------------------------------------------------------------- 2. small shapes
@pytest.mark.parametrize("radius,kind", SS.TWOVIEW_KINDS, ids=["r5-geodesic", "r2-adaptive"])
@pytest.mark.parametrize("shape", SS.TWOVIEW_SHAPES, ids=SS.shape_id)
def test_small_shapes_run_the_kernel(hip_ctx, shape, radius, kind):
    """every tiny and thin shape, the tile edges 31/32/33 and 63/64/65 among them: the kernel runs (it never declines to the
    lists for a view's size) and gives the lists' and the restatement's bits"""
    w, h, D = shape
    assert set(SS.TILE_EDGE_WIDTHS) <= {s[0] for s in SS.TWOVIEW_SHAPES}
    case = SS.small_twoview(w, h, D, radius, kind)
    imgs, ocams, op = cases.oracle_inputs(case)
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    want = _restated_maps(imgs, ocams, op)
    got, lists = _dense_and_lists(hip_ctx, p)
    for d in range(2):
        tag = "%s direction %d" % (case["name"], d)
        _assert_same(got[d][0], lists[d][0], tag + " against the lists")
        _assert_same(got[d][0], want[d], tag + " against the restatement")
        assert got[d][1]["n_eval"] == lists[d][1]["n_eval"], tag


@pytest.mark.parametrize("shape", [(33, 9, 40), (65, 12, 8)], ids=SS.shape_id)
def test_small_shapes_with_masks(hip_ctx, shape):
    w, h, D = shape
    case = SS.small_twoview(w, h, D, 5, 1, masks=True)
    imgs, ocams, op = cases.oracle_inputs(case)
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    want = _restated_maps(imgs, ocams, op)
    got, lists = _dense_and_lists(hip_ctx, p)
    for d in range(2):
        _assert_same(got[d][0], lists[d][0], "%s direction %d against the lists" % (case["name"], d))
        _assert_same(got[d][0], want[d], "%s direction %d against the restatement" % (case["name"], d))


# ---------------------------------------------------------------- 3. a wide view
def _ragged(h, w, seed):
    """60 % of a mask cleared in ragged runs: most candidate windows hold a masked tap"""
    rng = np.random.default_rng(seed)
    keep = np.ones((h, w), bool)
    for y in range(h):
        x = 0
        while x < w:
            run = int(rng.integers(1, 40))
            if rng.random() < 0.6:
                keep[y, x:x + run] = False
            x += run
    return keep.astype(np.uint8)


@pytest.mark.parametrize("ragged", [False, True], ids=["plain", "ragged_mask"])
def test_one_wide_view(hip_ctx, ragged):
    """1920 x 48 x 256, geodesic r = 5: a full-width chunk, 60 tile columns, items of 32 (two of 16), 8 and 4 rows
    (StripItems::cut(48) = 32 + 8 + 2 x 4).  Ragged: the other view's mask mostly cleared, so that the select-form work list
    is long"""
    case = SS.small_twoview(1920, 48, 256, 5, 1)
    if ragged:
        views = list(case["views"])
        views[1] = (views[1][0], _ragged(48, 1920, 0x5AD0DE45),) + tuple(views[1][2:])
        case = dict(case, views=views)
        assert 0.3 < views[1][1].mean() < 0.5
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    with _options(hip_ctx, cost=capi.COST_CENSUS, census_dense=1):
        hip_ctx.twoview_wta(0, 1, p)
        st = hip_ctx.stats()
        assert st["used_dense_path"] and st["used_strip_kernel"], st
        got = hip_ctx.download_depth(0)
    with _options(hip_ctx, cost=capi.COST_CENSUS, census_dense=0):
        hip_ctx.twoview_wta(0, 1, p)
        st0 = hip_ctx.stats()
        assert not st0["used_dense_path"]
        lists = hip_ctx.download_depth(0)
    _assert_same(got, lists, "wide view%s against the lists" % (" (ragged mask)" if ragged else ""))
    assert st["n_eval"] == st0["n_eval"]
    assert np.isfinite(got).mean() > (0.02 if ragged else 0.2)


# ---------------------------------------------------------------- 4. bands and row ranges
def test_row_ranges_and_small_budget(hip_ctx):
    case, imgs, ocams, op, cams, p = _case("geodesic_masks", w=96, h=64, D=20)
    cases.upload_case(hip_ctx, case, cams)
    with _options(hip_ctx, cost=capi.COST_CENSUS, census_dense=1):
        hip_ctx.twoview_wta(0, 1, p)
        st = hip_ctx.stats()
        assert st["used_dense_path"] and st["used_strip_kernel"]
        full = hip_ctx.download_depth(0)
        _assert_same(full, CR.twoview_wta_census(imgs[0], imgs[1], ocams[0], ocams[1], op), "one band")
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


# ---------------------------------------------------------------- 5. cost rows
@pytest.mark.parametrize("name", ["geodesic_masks", "adaptive_rect", "geodesic_r2"])
def test_cost_rows_value_by_value(hip_ctx, name):
    case, imgs, ocams, op, cams, p = _case(name)
    cases.upload_case(hip_ctx, case, cams)
    h, w = case["views"][0][0].shape[:2]
    never = np.uint64(0xFFFFFFFFFFFFFFFF)
    for ref, oth in DIRECTIONS:
        with _options(hip_ctx, cost=capi.COST_CENSUS, census_dense=1):
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
        dev = hip_ctx.twoview_pair_costs(ref, oth, p, xy, capi.COST_CENSUS)
        _assert_same(got, dev, "%s %d>%d cost rows against the device's pair costs" % (name, ref, oth))
        want = CR.pair_costs_census(imgs[ref], imgs[oth], op, xy)
        _assert_costs(got, want, "%s %d>%d cost rows against the restatement" % (name, ref, oth), op.bad_ret)
        assert (got[got != op.bad_ret] >= 0).all() and (got[got != op.bad_ret] <= 62).all()
    with _options(hip_ctx, cost=capi.COST_CENSUS, census_dense=1):
        for form in (3, 5, 1, 2):
            with pytest.raises(capi.StereoHipError):
                hip_ctx.twoview_cost_rows(0, 1, p, 0, 4, form)
    with _options(hip_ctx, cost=capi.COST_CENSUS, census_dense=0):
        with pytest.raises(capi.StereoHipError):
            hip_ctx.twoview_cost_rows(0, 1, p, 0, 4, 0)


# ---------------------------------------------------------------- 6. fall-backs
@pytest.mark.parametrize("name,over,extra", [
    ("geodesic_rect", dict(radius=3), dict()),
    ("adaptive_rect", dict(w=400, h=24, D=330), dict()),                      # cstride + 32 > 320: wider than the chunk
    ("geodesic_rect", dict(), dict(force_generic=1)),
    ("adaptive_verged", dict(radius=5), dict()),
    ("adaptive_verged", dict(w=72, h=44, D=20, radius=2), dict(force_dense=1)),  # proposed, refuted by the scan, redone
], ids=["radius_3", "wider_than_the_chunk", "force_generic", "verged", "force_dense_refuted"])
def test_fall_backs(hip_ctx, name, over, extra):
    case, imgs, ocams, op, cams, p = _case(name, **over)
    cases.upload_case(hip_ctx, case, cams)
    with _options(hip_ctx, cost=capi.COST_CENSUS, census_dense=0):
        lists = _passes(hip_ctx, p, False)
    with _options(hip_ctx, cost=capi.COST_CENSUS, census_dense=1, **extra):
        got = _passes(hip_ctx, p, False)
        if name == "adaptive_rect":
            with pytest.raises(capi.StereoHipError):
                hip_ctx.twoview_cost_rows(0, 1, p, 0, 4, 0)
    want = _restated_maps(imgs, ocams, op)
    for d in range(2):
        _assert_same(got[d][0], lists[d][0], "%s %s direction %d against the lists" % (name, extra, d))
        _assert_same(got[d][0], want[d], "%s %s direction %d against the restatement" % (name, extra, d))


def test_the_option_changes_nothing_under_ncc_and_sad(hip_ctx):
    case, imgs, ocams, op, cams, p = _case("geodesic_masks")
    cases.upload_case(hip_ctx, case, cams)
    for opts in (dict(cost=capi.COST_NCC), dict(cost=capi.COST_SAD), dict(cost=capi.COST_SAD, sad_dense=1)):
        runs = []
        for census_dense in (0, 1):
            with _options(hip_ctx, census_dense=census_dense, **opts):
                maps = []
                for ref, oth in DIRECTIONS:
                    hip_ctx.twoview_wta(ref, oth, p)
                    st = hip_ctx.stats()
                    maps.append((hip_ctx.download_depth(ref), st["used_dense_path"], st["used_strip_kernel"], st["n_eval"]))
                runs.append(maps)
        for d in range(2):
            _assert_same(runs[1][d][0], runs[0][d][0], "%s direction %d" % (opts, d))
            assert runs[1][d][1:] == runs[0][d][1:], (opts, d)


# ---------------------------------------------------------------- 7. state
def test_switching_on_one_context_reupload_and_mask_change(hip_ctx):
    case, imgs, ocams, op, cams, p = _case("geodesic_rect")
    cases.upload_case(hip_ctx, case, cams)
    ncc1 = hip_ctx.twoview_compute(0, 1, p)
    with _options(hip_ctx, cost=capi.COST_CENSUS, census_dense=1):
        census_dense = hip_ctx.twoview_compute(0, 1, p)
        st = hip_ctx.stats()
        assert st["used_dense_path"] and st["used_strip_kernel"]
    with _options(hip_ctx, cost=capi.COST_SAD, sad_dense=1):
        sad_dense = hip_ctx.twoview_compute(0, 1, p)
        st = hip_ctx.stats()
        assert st["used_dense_path"] and st["used_strip_kernel"]
    with _options(hip_ctx, cost=capi.COST_CENSUS):
        census_lists = hip_ctx.twoview_compute(0, 1, p)
        assert not hip_ctx.stats()["used_dense_path"]
    ncc2 = hip_ctx.twoview_compute(0, 1, p)
    for k in range(2):
        _assert_same(ncc2[k], ncc1[k], "ncc again %d" % k)
        _assert_same(census_dense[k], census_lists[k], "census dense against lists %d" % k)
        assert not CR.same_bits(census_dense[k], ncc1[k]) and not CR.same_bits(census_dense[k], sad_dense[k])
    # another image into the same slots: the padded planes of the old one must not survive
    case2, imgs2, ocams2, op2, cams2, p2 = _case("geodesic_masks")
    cases.upload_case(hip_ctx, case2, cams2)
    got, lists = _dense_and_lists(hip_ctx, p2)
    want = _restated_maps(imgs2, ocams2, op2)
    for d in range(2):
        _assert_same(got[d][0], lists[d][0], "after the re-upload, direction %d against the lists" % d)
        _assert_same(got[d][0], want[d], "after the re-upload, direction %d against the restatement" % d)
    # the same images under other masks: likewise
    views = [(v[0], np.ascontiguousarray(v[1][:, ::-1]),) + tuple(v[2:]) for v in case2["views"]]
    assert not np.array_equal(views[0][1], case2["views"][0][1])
    case3 = dict(case2, views=views)
    cases.upload_case(hip_ctx, case3, cams2)
    got3, lists3 = _dense_and_lists(hip_ctx, p2)
    for d in range(2):
        _assert_same(got3[d][0], lists3[d][0], "after the mask change, direction %d against the lists" % d)
        assert not CR.same_bits(got3[d][0], got[d][0])


def test_compute_with_cross_check_either_overlap(hip_ctx):
    case, imgs, ocams, op, cams, p = _case("geodesic_rect")
    cases.upload_case(hip_ctx, case, cams)
    dl, dr = O.twoview_cross_check(ocams[0], ocams[1], op, *_restated_maps(imgs, ocams, op))
    for ov in (1, 0):
        with _options(hip_ctx, cost=capi.COST_CENSUS, census_dense=1, tv_overlap=ov):
            gl, gr = hip_ctx.twoview_compute(0, 1, p)
            st = hip_ctx.stats()
        assert st["used_dense_path"] and st["used_strip_kernel"], (ov, st)
        _assert_same(gl, dl, "tv_overlap %d left" % ov)
        _assert_same(gr, dr, "tv_overlap %d right" % ov)
        assert np.isfinite(gl).sum() > 0 and np.isinf(gl).sum() + np.isnan(gl).sum() > 0
    flags = capi.FILTER_GAPS | capi.FILTER_MEDIAN
    fl = F.filter_map(case["views"][0][0], case["views"][0][1], dl, F.oparams(p), flags)
    fr = F.filter_map(case["views"][1][0], case["views"][1][1], dr, F.oparams(p), flags)
    with _options(hip_ctx, cost=capi.COST_CENSUS, census_dense=1, filter_invalid=flags):
        gl, gr = hip_ctx.twoview_compute(0, 1, p)
        st = hip_ctx.stats()
    assert st["used_dense_path"] and st["used_strip_kernel"], st
    _assert_same(gl, fl, "filtered left")
    _assert_same(gr, fr, "filtered right")


# ---------------------------------------------------------------- 8. behind the scan
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.mark.parametrize("name", ["geodesic_masks", "geodesic_r2"])
def test_wta_outputs_and_subpixel_behind_the_dense_scan(hip_ctx, name):
    case, imgs, ocams, op, cams, p = _case(name)
    cases.upload_case(hip_ctx, case, cams)
    for ref, oth in DIRECTIONS:
        runs = []
        for census_dense in (1, 0):
            with _options(hip_ctx, cost=capi.COST_CENSUS, census_dense=census_dense, wta_outputs=3):
                hip_ctx.twoview_wta(ref, oth, p)
                st = hip_ctx.stats()
                out = dict(depth=hip_ctx.download_depth(ref))
                out.update(hip_ctx.wta_outputs(ref))
            assert bool(st["used_dense_path"]) == bool(census_dense) and bool(st["used_strip_kernel"]) == bool(census_dense), st
            with _options(hip_ctx, cost=capi.COST_CENSUS, census_dense=census_dense, wta_outputs=3, subpixel=1):
                hip_ctx.twoview_wta(ref, oth, p)
                st = hip_ctx.stats()
                sub = dict(refined=hip_ctx.download_depth(ref))
                sub.update(hip_ctx.subpixel(ref))
            assert bool(st["used_dense_path"]) == bool(census_dense) and bool(st["used_strip_kernel"]) == bool(census_dense), st
            out.update(sub)
            runs.append(out)
        assert set(runs[0]) == set(runs[1]) and {"win_xy", "runner_xy", "min_cost", "second_cost", "delta"} <= set(runs[0])
        for k in sorted(runs[0]):
            a, b = _bits(runs[0][k]), _bits(runs[1][k])
            assert np.array_equal(a, b), "%s %d>%d: %s differs at %d places" % (name, ref, oth, k, (a != b).sum())
        assert np.isfinite(runs[0]["min_cost"]).any() and (runs[0]["delta"] != 0).any()


# ---------------------------------------------------------------- 9. constants
CONSTANTS = [e for e in CC.ENTRIES + CC.SAD_ENTRIES
             if e.case in CC.RECTIFIED and set(dict(e.over)) & {"weight_cutoff", "bad_ret", "wta_margin", "second_best_factor"}]


@pytest.mark.parametrize("e", CONSTANTS, ids=CC.entry_id)
def test_away_from_the_default_constants(hip_ctx, e):
    case = CC.build(e)
    cams, p = cases.hip_inputs(case)
    for k, v in e.over:
        assert getattr(p, k) == v
    cases.upload_case(hip_ctx, case, cams)
    got, lists = _dense_and_lists(hip_ctx, p)
    for d in range(2):
        _assert_same(got[d][0], lists[d][0], "%s direction %d against the lists" % (CC.entry_id(e), d))
        assert got[d][1]["n_eval"] == lists[d][1]["n_eval"]


def test_the_constants_table_moves_all_four():
    moved = set()
    for e in CONSTANTS:
        moved |= set(dict(e.over))
    assert {"weight_cutoff", "bad_ret", "wta_margin", "second_best_factor"} <= moved


# ---------------------------------------------------------------- 10. the host class's setter
def test_host_class_setter(hip_ctx, tmp_path):
    import test_gpu_host_api as HA
    subprocess.check_call(["make", "-C", HA.HOST], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "host_census_dense_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + HA.HOST,
                           os.path.join(ROOT, "tests", "host_census_dense_test.cpp"),
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
    for on in (0, 1):
        outp = str(tmp_path / ("out%d.bin" % on))
        subprocess.check_call([exe, inp, outp, str(on)])
        (gl, gr), steps = HA._read_output(outp, 2, w, h)
        assert steps == [1, 3, 5, 8]
        _assert_same(gl, want[0], "host left, setCensusDense(%d)" % on)
        _assert_same(gr, want[1], "host right, setCensusDense(%d)" % on)
