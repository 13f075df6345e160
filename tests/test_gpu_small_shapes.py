"""Every stereo path of the library on tiny and thin views (tests/small_shapes.py): images narrower or shorter than their
own support window (every window cut by two opposite image edges at once), narrower than one tile of any kernel, with
more candidates than columns (the dense plan's cstride clamp), and widths on the tile edges 31/32/33 and 63/64/65 at
heights of 1 .. 13.  One test is one shape.

Tolerances are the project's own: 1e-9 relative against the CPU oracle (the device exp differs from libm's), bit equality
between device paths, e0 of capi.cert_bound for the fused cost rows."""
import contextlib
import ctypes as C
import functools
import math
import types

import numpy as np
import pytest

import cases
import oracle_ffi as O
import sad_ref as S
import small_shapes as SS
import test_gpu_cert_rows as CR
import test_gpu_twoview_mrf as TM
import test_gpu_wta_outputs as WO
import twoview_mrf_ref as MR
from stereoreconstruction_amd import capi

pytestmark = pytest.mark.gpu

DIRECTIONS = ((0, 1), (1, 0))
KIND_IDS = ["r%d_%s" % (r, "geodesic" if k else "adaptive") for r, k in SS.TWOVIEW_KINDS]
FROM_5X5 = SS.TWOVIEW_SHAPES[SS.TWOVIEW_SHAPES.index((5, 5, 3)):]
# options tests/test_gpu_wta_outputs.py's _options does not know
EXTRA_DEFAULTS = dict(geodma=1, mvs_staged=1, mvs_async=1)


def _shapes(shapes):
    return pytest.mark.parametrize("shape", shapes, ids=SS.shape_id)


kinds = pytest.mark.parametrize("radius,kind", SS.TWOVIEW_KINDS, ids=KIND_IDS)
masked = pytest.mark.parametrize("masks", [False, True], ids=["plain", "masks"])


@contextlib.contextmanager
def _options(ctx, **opts):
    extra = {k: opts.pop(k) for k in list(opts) if k in EXTRA_DEFAULTS}
    try:
        for k, v in extra.items():
            ctx.set_option(k, v)
        with WO._options(ctx, **opts):
            yield
    finally:
        for k in extra:
            ctx.set_option(k, EXTRA_DEFAULTS[k])


@functools.lru_cache(maxsize=None)
def _case(shape, radius, kind, masks=False, general=False):
    return case_inputs(SS.small_twoview(*shape, radius, kind, masks=masks, verged=general, distortion=general))


def case_inputs(case):
    """a case dict with its oracle and library inputs (tests/test_gpu_rigs.py builds its cases with this too)"""
    imgs, ocams, op = cases.oracle_inputs(case)
    cams, p = cases.hip_inputs(case)
    h, w = case["views"][0][1].shape
    return types.SimpleNamespace(case=case, imgs=imgs, ocams=ocams, op=op, cams=cams, p=p, w=w, h=h,
                                 white=[v[1] == 1 for v in case["views"]], tag=case["name"])


def oracle_passes(c):
    """the CPU oracle's two passes on case `c`, (depth, diag) each"""
    out = [O.twoview_wta(c.imgs[r], c.imgs[o], c.ocams[r], c.ocams[o], c.op, want_diag=True) for r, o in DIRECTIONS]
    for d, diag in out:
        d.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle(shape, radius, kind, masks=False, general=False):
    """the CPU oracle's two passes, (depth, diag) each: computed once, shared, never written to"""
    return oracle_passes(_case(shape, radius, kind, masks, general))


def _upload(ctx, c):
    cases.upload_case(ctx, c.case, c.cams)


def _assert_depth(got, want, tag):
    ok, msg, _ = cases.compare_depth(got, want, 1e-9)
    assert ok, "%s: %s" % (tag, msg)


def _assert_bits(got, want, tag):
    assert S.same_bits(got, want), "%s: %s" % (tag, S.diff_report(got, want))


# ---------------------------------------------------------------------------------------------- a. whole maps
@masked
@kinds
@_shapes(SS.TWOVIEW_SHAPES)
def test_whole_maps_against_the_oracle(hip_ctx, shape, radius, kind, masks):
    c = _case(shape, radius, kind, masks)
    want = _oracle(shape, radius, kind, masks)
    _upload(hip_ctx, c)
    for k, (ref, oth) in enumerate(DIRECTIONS):
        hip_ctx.twoview_wta(ref, oth, c.p)
        got, st = hip_ctx.download_depth(ref), hip_ctx.stats()
        depth, diag = want[k]
        print("%s %d>%d: finite %d, +INF %d, NaN %d, n_eval %d / %d" % (c.tag, ref, oth, np.isfinite(got).sum(), np.isposinf(got).sum(),
                                                                       np.isnan(got).sum(), st["n_eval"], diag["n_eval"]))
        _assert_depth(got, depth, "%s %d>%d" % (c.tag, ref, oth))
        assert st["n_eval"] == diag["n_eval"], "%s %d>%d" % (c.tag, ref, oth)
    if shape[0] == 1:
        assert np.isnan(got).all() and st["n_eval"] == 0            # one column: no candidate right to left


# ---------------------------------------------------------------------------------------------- b. every rectified path
def _strip(st):
    return WO._dense(st) and st["used_strip_kernel"]


# option "geodma" is read only where the windows leave in the strip kernel's layout (run_weights, csrc/srh_api.hip), and
# views this small take the strip kernel only when it is forced: geodma = 0 is run under strip = 4 and strip = 8
PATHS = WO.RECT_PATHS + [("geodma 0 strip 4", dict(geodma=0, strip=4), _strip), ("geodma 0 strip 8", dict(geodma=0, strip=8), _strip)]
# which windows kernel a path has to launch at r = 5 geodesic (names of Context.profile()): (ran, did not run)
WINDOW_KERNELS = {
    "strip 4": ("geodesic_dma_kernel", "geodesic_reg_kernel"), "strip 8": ("geodesic_dma_kernel", "geodesic_reg_kernel"),
    "geodma 0 strip 4": ("geodesic_reg_kernel", "geodesic_dma_kernel"), "geodma 0 strip 8": ("geodesic_reg_kernel", "geodesic_dma_kernel"),
    "strip 0": ("geodesic_reg_kernel", "geodesic_dma_kernel"), "defaults": ("geodesic_reg_kernel", "geodesic_dma_kernel"),
}
GROUPS = ("w<=2r", "h<=2r", "D>w", "tile edge")
# (shape, radius, path) the library declines, by a rule of the TwoView pass driver (TvPass::plan, twoview_wta_run; csrc/srh_api.hip) quoted here; the depth maps
# and planes of a declined pair are still the walk kernel's bits
DECLINES = {
}


@kinds
@_shapes(SS.TWOVIEW_SHAPES)
def test_every_rectified_path_gives_the_walk_kernels_bits(hip_ctx, shape, radius, kind):
    check_every_rectified_path(hip_ctx, _case(shape, radius, kind), lambda tag: DECLINES.get((shape, radius, tag)),
                               windows=(radius, kind) == (5, 1))


def check_every_rectified_path(hip_ctx, c, declined, windows=False):
    """every entry of PATHS on case `c` against the walk kernel; declined(tag) -> the rule by which the driver declines the
    path on this case, or None; windows: check the windows kernel each path launches too (tests/test_gpu_rigs.py shares this)"""
    check_windows = windows
    _upload(hip_ctx, c)
    want = WO._yardstick(hip_ctx, c.p)
    for tag, opts, ran in PATHS:
        declines = declined(tag) is not None
        windows = WINDOW_KERNELS.get(tag) if check_windows and not declines else None
        with _options(hip_ctx, wta_outputs=3, **opts):
            for k, (ref, oth) in enumerate(DIRECTIONS):
                if windows:
                    hip_ctx.profile_reset()
                    hip_ctx.profile_enable(True)
                try:
                    d, got, st = WO._pass(hip_ctx, ref, oth, c.p)
                finally:
                    if windows:
                        hip_ctx.synchronize()
                        hip_ctx.profile_enable(False)
                what = "%s %s %d>%d" % (c.tag, tag, ref, oth)
                if windows:
                    launched = set(hip_ctx.profile().keys())
                    assert windows[0] in launched and windows[1] not in launched, "%s: windows by %s" % (what, sorted(k for k in launched if "geodesic" in k or "weights" in k))
                if declines:
                    assert not ran(st), "%s: listed as declined (%s), but the path ran: %s" % (what, declined(tag), st)
                else:
                    assert ran(st), "%s: the intended path did not run: %s" % (what, st)
                WO._same_planes(got, want[k][1], what)
                _assert_bits(d, want[k][0], what + " depth map")


def test_every_path_runs_in_every_shape_group():
    """with the test above (a pair that is not in DECLINES ran its kernel): no path is absent from a whole group"""
    for (shape, radius, tag), rule in DECLINES.items():
        assert shape in SS.TWOVIEW_SHAPES and tag in [t for t, _, _ in PATHS] and rule
    for radius, _ in SS.TWOVIEW_KINDS:
        for group in GROUPS:
            members = [s for s in SS.TWOVIEW_SHAPES if group in SS.groups(s, radius)]
            assert members, (radius, group)
            for tag, _, _ in PATHS:
                assert any((s, radius, tag) not in DECLINES for s in members), "path %r never runs at r = %d in group %s" % (tag, radius, group)


@kinds
def test_the_template_scan_runs_at_the_tile_edges(hip_ctx, radius, kind):
    """the `defaults` predicate above is content with walked tiles: here twoview_tscan_kernel has to settle tiles itself on
    either side of both tile edges (32: the cost tiles, 64: its own), and nothing at all with the option off"""
    settled = {}
    for shape in [s for s in SS.TWOVIEW_SHAPES if s[0] in SS.TILE_EDGE_WIDTHS]:
        c = _case(shape, radius, kind)
        _upload(hip_ctx, c)
        n = []
        for ref, oth in DIRECTIONS:
            hip_ctx.twoview_wta(ref, oth, c.p)
            st = hip_ctx.stats()
            assert WO._dense(st) and st["scan_tiles_template"] + st["scan_tiles_walked"] > 0, (c.tag, st)
            n.append(st["scan_tiles_template"])
        print("%s: tiles settled by the template scan %s of %d" % (c.tag, n, ((c.w + 63) // 64) * c.h))
        settled[shape[0]] = min(n)
    for edge in ((31, 32, 33), (63, 64, 65)):
        assert all(settled[w] > 0 for w in edge), "the template scan settled no tile at some width of %s: %s" % (edge, settled)
    with _options(hip_ctx, tscan=0):
        hip_ctx.twoview_wta(0, 1, c.p)
        assert hip_ctx.stats()["scan_tiles_template"] == 0


# ---------------------------------------------------------------------------------------------- c. planes
@masked
@kinds
@_shapes(FROM_5X5)
def test_planes_against_the_oracle(hip_ctx, shape, radius, kind, masks):
    c = _case(shape, radius, kind, masks)
    want = _oracle(shape, radius, kind, masks)
    _upload(hip_ctx, c)
    for k, (ref, oth) in enumerate(DIRECTIONS):
        diag = want[k][1]
        with _options(hip_ctx, wta_outputs=3):
            _, got, _ = WO._pass(hip_ctx, ref, oth, c.p)
        white = c.white[ref]
        agree = (got["win_xy"] == diag["win_xy"]).all(axis=2) & WO._close(got["min_cost"], diag["min_cost"]) & \
            WO._close(got["second_cost"], diag["second_cost"])
        bad = np.argwhere(~agree)
        print("%s %d>%d: %d of %d WHITE pixels disagree with the oracle" % (c.tag, ref, oth, len(bad), white.sum()))
        for y, x in bad:
            gap = WO._decision_gap(c.imgs, c.ocams, c.op, ref, oth, int(x), int(y))
            print("  (%d,%d): win %s / %s, min %r / %r, second %r / %r, decision gap %.3g" % (
                x, y, got["win_xy"][y, x], diag["win_xy"][y, x], got["min_cost"][y, x], diag["min_cost"][y, x],
                got["second_cost"][y, x], diag["second_cost"][y, x], gap))
            assert gap <= 1e-7, "%s %d>%d pixel (%d,%d): disagrees with the oracle, no decision within 1e-7 of flipping (gap %g)" % (c.tag, ref, oth, x, y, gap)
        assert len(bad) <= 0.01 * white.sum()
        # outside the mask: nothing
        assert (got["win_xy"][~white] == -1).all() and (got["runner_xy"][~white] == -1).all()
        assert np.isposinf(got["min_cost"][~white]).all() and np.isposinf(got["second_cost"][~white]).all()
        assert np.isfinite(got["min_cost"][got["win_xy"][..., 0] >= 0]).all()
        assert np.isfinite(got["second_cost"][got["runner_xy"][..., 0] >= 0]).all()
        assert np.isposinf(got["min_cost"][white & (got["win_xy"][..., 0] < 0)]).all()


# ---------------------------------------------------------------------------------------------- d. cost rows
def _rows_shapes(radius):
    return [s for s in SS.TWOVIEW_SHAPES if s[2] > s[0] or s[0] <= 2 * radius]


UP_TO_12X12 = SS.TWOVIEW_SHAPES[:SS.TWOVIEW_SHAPES.index((12, 12, 8)) + 1]
# ... and the larger shapes with D > w: at 40x3x64 the clamp `if (cstride > W + 8) cstride = (W + 8 + 7) & ~7` changes the stride
EXACT_ROWS_SHAPES = UP_TO_12X12 + [s for s in SS.TWOVIEW_SHAPES if s[2] > s[0] and s not in UP_TO_12X12]
ROWS_CASES = [(s, r, k) for r, k in SS.TWOVIEW_KINDS for s in _rows_shapes(r)]
ROWS_IDS = ["%s-%s" % (SS.shape_id(s), KIND_IDS[SS.TWOVIEW_KINDS.index((r, k))]) for s, r, k in ROWS_CASES]


@functools.lru_cache(maxsize=None)
def _oracle_rows(shape, radius, kind, masks):
    """sro_twoview_cost_ncc of every (pixel, column of the pixel's row) left to right: (h, w, w) float64"""
    c = _case(shape, radius, kind, masks)
    out = np.empty((c.h, c.w, c.w))
    L = O.lib()
    for y in range(c.h):
        for x in range(c.w):
            wts = np.ascontiguousarray(O.weights(c.imgs[0], x, y, c.op), dtype=np.float64)
            for cx in range(c.w):
                out[y, x, cx] = L.sro_twoview_cost_ncc(C.byref(c.imgs[0].c), C.byref(c.imgs[1].c), O.dptr(wts), C.byref(c.op), x, y, cx, y)
    out.setflags(write=False)
    return out


@masked
@pytest.mark.parametrize("strip", [0, 4, 8])
@pytest.mark.parametrize("shape,radius,kind", ROWS_CASES, ids=ROWS_IDS)
def test_fused_cost_rows_within_the_bound(hip_ctx, shape, radius, kind, strip, masks):
    """forms 5 and 3, raw and redone, against form 0 (tests/test_gpu_cert_rows.py); with masks a view this small may be left
    without a stored value, without them never"""
    c = _case(shape, radius, kind, masks)
    _upload(hip_ctx, c)
    tag = "%s strip=%d" % (c.tag, strip)
    worst, n_cert, n_clamp, n_unc = CR._rows_check(hip_ctx, c.p, 0, c.h, strip, tag)
    print("cost rows %s: max |fused - exact| = %.3g e0 over %d certified entries (%d clamps, %d uncertified)" % (tag, worst, n_cert, n_clamp, n_unc))
    # the bound is held over something: "certified" counts every stored value that is neither NaN nor the clamp -- on views
    # whose every window an image edge cuts these come from the select forms and the border instantiation (the reference's
    # arithmetic under every form), so the bound holds there with room; a fast-form candidate needs a whole window, w, h > 2r + 1
    if not masks:
        assert n_cert > 0, tag


@masked
@kinds
@_shapes(EXACT_ROWS_SHAPES)
def test_exact_cost_rows_against_the_oracle(hip_ctx, shape, radius, kind, masks):
    """every live entry of the rows in the reference's arithmetic is the oracle's cost of (pixel, lo + k), in all three
    kernel forms"""
    c = _case(shape, radius, kind, masks)
    _upload(hip_ctx, c)
    want_all = _oracle_rows(shape, radius, kind, masks)
    for strip in (0, 4, 8):
        tag = "%s strip=%d" % (c.tag, strip)
        hip_ctx.set_option("strip", strip)
        try:
            exact, rng, us = hip_ctx.twoview_cost_rows(0, 1, c.p, 0, c.h, 0)
        finally:
            hip_ctx.set_option("strip", 1)
        assert us == (strip != 0), tag
        nonempty = rng[..., 1] >= rng[..., 0]
        assert (rng[..., 0][nonempty] >= 0).all() and (rng[..., 1][nonempty] < c.w).all(), tag
        # the plan's stride (TvPass::plan): the widest range + margins in whole eights, clamped to the image's width + 8
        span = float(c.w) * c.p.image_scale * abs(1.0 / c.p.min_depth - 1.0 / c.p.max_depth)
        cstride = (math.ceil(span) + 3 + 7) & ~7
        if cstride > c.w + 8:
            cstride = (c.w + 8 + 7) & ~7
        assert exact.shape[2] == cstride, tag
        # (that restates the plan; what the stride has to do is hold every pixel's range, and the table has to keep a shape
        # on which the clamp changes it)
        assert (rng[..., 1] - rng[..., 0] + 1).max() <= exact.shape[2], tag
        if shape == (40, 3, 64):
            assert cstride == 48 < (math.ceil(span) + 3 + 7) & ~7 == 72, tag
        live = CR._valid(rng, exact.shape[2]) & (exact.view(np.uint64) != CR.UNWRITTEN)
        ys, xs, ks = np.nonzero(live)
        want = want_all[ys, xs, rng[ys, xs, 0] + ks]
        ok = WO._close(exact[ys, xs, ks], want)
        print("%s: cstride %d, %d live entries against the oracle, %d off" % (tag, exact.shape[2], len(ys), (~ok).sum()))
        assert ok.all(), "%s: %d of %d entries, first (y, x, k) %s: got %r want %r" % (
            tag, (~ok).sum(), len(ys), [int(a[~ok][0]) for a in (ys, xs, ks)], exact[ys, xs, ks][~ok][0], want[~ok][0])
        if c.w >= 2 and not masks:
            assert len(ys) > 0, tag


# ---------------------------------------------------------------------------------------------- e. SAD
@masked
@kinds
@_shapes(SS.TWOVIEW_SHAPES)
def test_sad_maps_on_both_plans(hip_ctx, shape, radius, kind, masks):
    check_sad_maps_on_both_plans(hip_ctx, _case(shape, radius, kind, masks))


def check_sad_maps_on_both_plans(hip_ctx, c):
    _upload(hip_ctx, c)
    want = [S.twoview_wta_sad(c.imgs[r], c.imgs[o], c.ocams[r], c.ocams[o], c.op) for r, o in DIRECTIONS]
    got = {}
    for sad_dense in (0, 1):
        with _options(hip_ctx, cost=capi.COST_SAD, sad_dense=sad_dense):
            for k, (ref, oth) in enumerate(DIRECTIONS):
                hip_ctx.twoview_wta(ref, oth, c.p)
                st = hip_ctx.stats()
                what = "%s sad_dense=%d %d>%d" % (c.tag, sad_dense, ref, oth)
                assert bool(st["used_dense_path"]) == bool(sad_dense), "%s: %s" % (what, st)
                got[sad_dense, k] = hip_ctx.download_depth(ref)
                _assert_bits(got[sad_dense, k], want[k], what)
    for k in range(2):
        _assert_bits(got[1, k], got[0, k], "%s dense against lists, pass %d" % (c.tag, k))


# ---------------------------------------------------------------------------------------------- f. rows one at a time
@pytest.mark.parametrize("opts", [dict(), dict(strip=8), dict(force_generic=1)], ids=["defaults", "strip8", "lists"])
@kinds
@_shapes([(9, 4, 8), (12, 12, 8), (33, 9, 40), (65, 12, 8)])
def test_rows_one_at_a_time_give_the_whole_pass(hip_ctx, shape, radius, kind, opts):
    check_row_bands_give_the_whole_pass(hip_ctx, _case(shape, radius, kind), opts)


def check_row_bands_give_the_whole_pass(hip_ctx, c, opts, bands=None):
    """`bands`: the (y0, y1) the pass is split into, every row on its own by default"""
    bands = [(y, y + 1) for y in range(c.h)] if bands is None else bands
    assert sorted(y for y0, y1 in bands for y in range(y0, y1)) == list(range(c.h))
    _upload(hip_ctx, c)
    blank = np.full((c.h, c.w), np.nan)
    for ref, oth in DIRECTIONS:
        with _options(hip_ctx, **opts):
            hip_ctx.twoview_wta(ref, oth, c.p)
            whole = hip_ctx.download_depth(ref)
            hip_ctx.upload_depth(ref, blank)
            assert np.isnan(hip_ctx.download_depth(ref)).all()
            for y0, y1 in bands:
                hip_ctx.twoview_wta(ref, oth, c.p, y0, y1)
            _assert_bits(hip_ctx.download_depth(ref), whole, "%s %s %d>%d in %d bands" % (c.tag, opts, ref, oth, len(bands)))
        assert not np.isnan(whole).all()


# ---------------------------------------------------------------------------------------------- g. both passes + cross-check
COMPUTE_CASES = [(s, False) for s in SS.TWOVIEW_SHAPES] + [(s, True) for s in ((5, 5, 3), (9, 4, 8), (33, 9, 40), (65, 12, 8))]


@kinds
@pytest.mark.parametrize("shape,masks", COMPUTE_CASES, ids=[SS.shape_id(s) + ("-masks" if m else "") for s, m in COMPUTE_CASES])
def test_compute_against_the_oracles_passes_and_cross_check(hip_ctx, shape, masks, radius, kind):
    check_compute(hip_ctx, _case(shape, radius, kind, masks), _oracle(shape, radius, kind, masks))


def check_compute(hip_ctx, c, oracle):
    (dl, _), (dr, _) = oracle
    want = O.twoview_cross_check(c.ocams[0], c.ocams[1], c.op, dl, dr)
    _upload(hip_ctx, c)
    for overlap in (1, 0):
        with _options(hip_ctx, tv_overlap=overlap):
            got = hip_ctx.twoview_compute(0, 1, c.p)
        for k in range(2):
            _assert_depth(got[k], want[k], "%s tv_overlap=%d map %d" % (c.tag, overlap, k))


# ---------------------------------------------------------------------------------------------- h. general geometry
@pytest.mark.parametrize("radius,kind", [(2, 1), (5, 0)], ids=["r2_geodesic", "r5_adaptive"])
@_shapes([(5, 5, 3), (9, 7, 8), (12, 9, 8), (33, 7, 12), (65, 6, 8)])
def test_general_geometry(hip_ctx, shape, radius, kind):
    c = _case(shape, radius, kind, True, True)
    want = _oracle(shape, radius, kind, True, True)
    _upload(hip_ctx, c)
    walk = WO._yardstick(hip_ctx, c.p)
    for k in range(2):
        _assert_depth(walk[k][0], want[k][0], "%s walk kernel, pass %d" % (c.tag, k))
    for tag, opts, ran in WO.GENERAL_PATHS:
        with _options(hip_ctx, wta_outputs=3, **opts):
            for k, (ref, oth) in enumerate(DIRECTIONS):
                d, got, st = WO._pass(hip_ctx, ref, oth, c.p)
                what = "%s %s %d>%d" % (c.tag, tag, ref, oth)
                assert ran(st), "%s: the intended path did not run: %s" % (what, st)
                _assert_depth(d, want[k][0], what)
                WO._same_planes(got, walk[k][1], what)
                _assert_bits(d, walk[k][0], what + " depth map")


# ---------------------------------------------------------------------------------------------- i. MultiViewStereo
@functools.lru_cache(maxsize=None)
def _mvs(shape, kind, distortion):
    case = SS.small_mvs(*shape, kind, distortion)
    imgs, ocams, op = cases.oracle_inputs(case)
    neigh = [[int(n) for n in v] for v in O.mvs_neighbours(ocams, op)]
    want = [O.mvs_initial_estimate(imgs, ocams, v, neigh[v], op, want_peaks=True) for v in range(3)]
    for d, pk, _ in want:
        d.setflags(write=False)
        pk.setflags(write=False)
    cams, p = cases.hip_inputs(case)
    return types.SimpleNamespace(case=case, imgs=imgs, ocams=ocams, op=op, cams=cams, p=p, neigh=neigh, want=want, tag=case["name"])


@pytest.mark.parametrize("kind,distortion", SS.MVS_KINDS, ids=["geodesic", "adaptive_distorted"])
@_shapes(SS.MVS_SHAPES)
def test_mvs(hip_ctx, shape, kind, distortion):
    c = _mvs(shape, kind, distortion)
    w, h = shape[0], shape[1]
    assert capi.mvs_neighbours(c.cams, c.p) == c.neigh
    _upload(hip_ctx, c)
    for v in range(3):
        hip_ctx.mvs_initial_estimate(v, c.neigh[v], c.p)
        got = hip_ctx.download_depth(v)
        _assert_depth(got, c.want[v][0], "%s view %d" % (c.tag, v))
        n_eval = hip_ctx.stats()["n_eval"]
        for opt, val in (("force_generic", 1), ("mvs_staged", 0), ("mvs_async", 0)):
            with _options(hip_ctx, **{opt: val}):
                hip_ctx.mvs_initial_estimate(v, c.neigh[v], c.p)
                _assert_bits(hip_ctx.download_depth(v), got, "%s view %d under %s=%d" % (c.tag, v, opt, val))
                assert hip_ctx.stats()["n_eval"] == n_eval
    # the cross-check in view order, each view reading the already filtered earlier views
    ref = [np.array(d) for d, _, _ in c.want]
    for v in range(3):
        O.mvs_cross_check(c.imgs, c.ocams, v, c.op, ref)
    for v in range(3):
        hip_ctx.upload_depth(v, np.array(c.want[v][0]))
    for v in range(3):
        hip_ctx.mvs_cross_check([0, 1, 2], v, c.p)
    for v in range(3):
        _assert_depth(hip_ctx.download_depth(v), ref[v], "%s view %d cross-check" % (c.tag, v))
    if SS.MVS_SHAPES.index(shape) >= SS.MVS_SHAPES.index((9, 7, 8)):
        # the sorted top-K (cost, depth) lists of view 0, as tests/test_gpu_edge_cases.py holds them to the oracle
        import torch
        depth, want_pk, _ = c.want[0]
        pk = torch.zeros((h, w, c.p.top_k, 2), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        hip_ctx.mvs_initial_estimate(0, c.neigh[0], c.p, peaks_dev=pk.data_ptr())
        hip_ctx.synchronize()
        got = pk.cpu().numpy()
        assert np.allclose(got[..., 0], want_pk[..., 0], rtol=0, atol=1e-12), c.tag
        assert np.allclose(got[..., 1], want_pk[..., 1], rtol=1e-9, atol=0), c.tag
        _assert_depth(hip_ctx.download_depth(0), depth, c.tag + " with peaks")
        # the inline kernel, and the gathering kernel's top-K form for every wave (mvs_list_cost_kernel<2, true>)
        for opt in ("force_generic", "mvs_staged"):
            pk2 = torch.full((h, w, c.p.top_k, 2), 7.0, dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            with _options(hip_ctx, **{opt: 1 if opt == "force_generic" else 0}):
                hip_ctx.mvs_initial_estimate(0, c.neigh[0], c.p, peaks_dev=pk2.data_ptr())
                hip_ctx.synchronize()
            assert np.array_equal(got.view(np.uint64), pk2.cpu().numpy().view(np.uint64)), (c.tag, opt)


@pytest.mark.parametrize("kind,distortion", SS.MVS_KINDS, ids=["geodesic", "adaptive_distorted"])
def test_mvs_staged_and_gathering_kernels_both_take_waves(hip_ctx, kind, distortion):
    """"staged gives the gathering kernel's bits" (test_mvs) compares two kernels only where the staged one takes a wave: a
    window box over an image border goes to the gathering kernel, which on the smallest views is every window.  Tallied over
    the table: some shapes stage waves under the defaults, none does under mvs_staged = 0 (the walk kernel then makes no
    window descriptors and counts neither kind), and no window fits a 3x3 view."""
    staged = {}
    for shape in SS.MVS_SHAPES:
        c = _mvs(shape, kind, distortion)
        _upload(hip_ctx, c)
        tally = [0, 0, 0]
        for v in range(3):
            hip_ctx.mvs_initial_estimate(v, c.neigh[v], c.p)
            st = hip_ctx.stats()
            tally[0] += st["mvs_waves_staged"]
            tally[1] += st["mvs_waves_listed"]
            with _options(hip_ctx, mvs_staged=0):
                hip_ctx.mvs_initial_estimate(v, c.neigh[v], c.p)
                st = hip_ctx.stats()
                assert st["mvs_waves_staged"] == 0, (c.tag, v, st)
                tally[2] += st["mvs_waves_listed"]
        print("%s: waves staged %d, listed %d; with mvs_staged = 0 listed %d" % ((c.tag,) + tuple(tally)))
        staged[shape] = tally[0]
    assert staged[(3, 3, 4)] == 0, staged                              # no 5 x 5 window box fits a 3 x 3 image
    # (the table's one shape with staged waves is 8x8, two waves of view pairs whose boxes lie inside the image; everywhere
    # else the boxes reach a border and test_mvs compares the gathering kernel with itself.  With distorted neighbours the
    # boxes move, so that variant is tallied only.)
    if not distortion:
        assert sum(n > 0 for n in staged.values()) >= 1, staged


# ---------------------------------------------------------------------------------------------- j. label costs
@kinds
@_shapes([(5, 5, 3), (9, 4, 8), (33, 9, 40)])
def test_label_costs(hip_ctx, shape, radius, kind):
    check_label_costs(hip_ctx, _case(shape, radius, kind))


def check_label_costs(hip_ctx, c):
    _upload(hip_ctx, c)
    fill = MR.fill_value(c.p.window_radius, c.p.bad_ret)
    for ref, oth in DIRECTIONS:
        want_pix = TM._cpu_label_pixels(c.case, c.ocams, c.op, ref, oth)
        has = want_pix[..., 0] != TM.NONE
        assert has.any()
        yy, xx, dd = np.nonzero(has)
        xy = np.stack([xx, yy, want_pix[yy, xx, dd, 0], want_pix[yy, xx, dd, 1]], 1).astype(np.int32)
        for cost_kind, kname in ((capi.COST_NCC, "ncc"), (capi.COST_SAD, "sad")):
            tag = "%s %s %d>%d" % (c.tag, kname, ref, oth)
            with _options(hip_ctx, cost=cost_kind):
                cost, pix = hip_ctx.twoview_label_costs(ref, oth, c.p)
                assert np.array_equal(pix, want_pix), "%s: %d label pixels differ" % (tag, (pix != want_pix).any(axis=-1).sum())
                assert (cost[~has] == fill).all(), tag
                pc = hip_ctx.twoview_pair_costs(ref, oth, c.p, xy, cost_kind)
                _assert_bits(cost[yy, xx, dd], pc, tag + " vs pair costs")
                for y in range(c.h):
                    band, bpix = hip_ctx.twoview_label_costs(ref, oth, c.p, y, y + 1)
                    _assert_bits(band, cost[y:y + 1], "%s row %d" % (tag, y))
                    assert np.array_equal(bpix, pix[y:y + 1]), "%s row %d" % (tag, y)
