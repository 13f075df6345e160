"""The dense plan (rig_is_row_aligned, TvPass::plan, pixel_range_kernel, the strip, per-tile and fused cost kernels, the
template scan's three tiers, the certified redo, the SAD strip kernel) on the row-aligned rigs of tests/rig_cases.py: rotated,
displaced, far from the origin, scaled, slots exchanged, a baseline just inside the rig test's tolerance, one cx or one fx per
view, off-axis and anamorphic intrinsics, a metric baseline -- and two rigs the rig test turns away.  Everything else that
reaches the dense plan builds its cameras with synthetic.rectified_cameras (K shared, R = I, C_left = 0), on which R*point is
exact, the |src| terms of the template scan's bound vanish, the template is an exact shift, the candidates lie on one side
of x and no label projects onto an integer column.  One test is one rig at 100 x 24 x 24.

Tolerances are the project's own: 1e-9 relative against the CPU oracle, bit equality between device paths, e0 of
capi.cert_bound for the fused cost rows.  The checks themselves are those of tests/test_gpu_small_shapes.py,
tests/test_gpu_wta_outputs.py, tests/test_gpu_cert_rows.py, tests/test_gpu_tscan_bound.py and tests/test_gpu_subpixel.py,
shared, not restated."""
import ctypes as C
import functools

import numpy as np
import pytest

import cases
import oracle_ffi as O
import rig_cases as RC
import test_gpu_cert_rows as CR
import test_gpu_small_shapes as SM
import test_gpu_subpixel as SP
import test_gpu_tscan_bound as TB
import test_gpu_wta_outputs as WO
from stereoreconstruction_amd import capi

pytestmark = pytest.mark.gpu

DIRECTIONS = SM.DIRECTIONS
KINDS = [(5, 1), (2, 0)]
KIND_IDS = ["r5_geodesic", "r2_adaptive"]
kinds = pytest.mark.parametrize("radius,kind", KINDS, ids=KIND_IDS)
masked = pytest.mark.parametrize("masks", [False, True], ids=["plain", "masks"])
WALKED = ("half_pixel", "fx_ratio")                   # proposed, but the template serves (next to) no pixel


@functools.lru_cache(maxsize=None)
def _case(name, radius=5, kind=1, masks=False):
    return SM.case_inputs(RC.rig_twoview(name, radius=radius, kind=kind, masks=masks))


@functools.lru_cache(maxsize=None)
def _oracle(name, radius=5, kind=1, masks=False):
    """the CPU oracle's two passes, (depth, diag) each: computed once, shared, never written to"""
    return SM.oracle_passes(_case(name, radius, kind, masks))


# ---------------------------------------------------------------------------------------------- a. whole maps
@masked
@kinds
@pytest.mark.parametrize("name", list(RC.RIGS))
def test_whole_maps_against_the_oracle(hip_ctx, name, radius, kind, masks):
    c = _case(name, radius, kind, masks)
    want = _oracle(name, radius, kind, masks)
    SM._upload(hip_ctx, c)
    for k, (ref, oth) in enumerate(DIRECTIONS):
        hip_ctx.twoview_wta(ref, oth, c.p)
        got, st = hip_ctx.download_depth(ref), hip_ctx.stats()
        depth, diag = want[k]
        what = "%s %d>%d" % (c.tag, ref, oth)
        print("%s: finite %d, +INF %d, NaN %d, n_eval %d / %d, dense %d, tiles bound %d template %d walked %d" % (
            what, np.isfinite(got).sum(), np.isposinf(got).sum(), np.isnan(got).sum(), st["n_eval"], diag["n_eval"],
            st["used_dense_path"], st["scan_tiles_bound"], st["scan_tiles_template"], st["scan_tiles_walked"]))
        SM._assert_depth(got, depth, what)
        assert st["n_eval"] == diag["n_eval"], what
        # a proposed plan has to STAND (half_pixel and fx_ratio included), not be redone on the general kernels
        assert st["used_dense_path"] == RC.RIGS[name]["proposed"], (what, st)
        assert np.isfinite(got).any(), what


# ---------------------------------------------------------------------------------------------- b. every rectified path
# (rig, radius, path) the library declines, by a rule of the TwoView pass driver (TvPass::plan, csrc/srh_api.hip) quoted
# here; the depth maps and planes of a declined pair are still the walk kernel's bits
DECLINES = {
}


@kinds
@pytest.mark.parametrize("name", RC.PROPOSED)
def test_every_rectified_path_gives_the_walk_kernels_bits(hip_ctx, name, radius, kind):
    SM.check_every_rectified_path(hip_ctx, _case(name, radius, kind), lambda tag: DECLINES.get((name, radius, tag)))


def test_every_path_runs_on_some_rig():
    """with the test above (a pair that is not in DECLINES ran its kernel): no path is absent from every rig of a kind"""
    for (name, radius, tag), rule in DECLINES.items():
        assert name in RC.PROPOSED and tag in [t for t, _, _ in SM.PATHS] and rule
    for radius, _ in KINDS:
        for tag, _, _ in SM.PATHS:
            assert any((name, radius, tag) not in DECLINES for name in RC.PROPOSED), "path %r never runs at r = %d" % (tag, radius)


# ---------------------------------------------------------------------------------------------- c. tiers
@pytest.mark.parametrize("name", RC.PROPOSED)
def test_tiers(hip_ctx, name):
    """who settles the scan tiles: the per-pixel bound where the table says the template serves every pixel, the curve walk
    on half_pixel and fx_ratio -- and whoever does, the same bits and counts"""
    for (radius, kind), kid in zip(KINDS, KIND_IDS):
        c = _case(name, radius, kind)
        SM._upload(hip_ctx, c)
        for arith in (capi.ARITH_CERTIFIED, capi.ARITH_EXACT):
            what = "%s arith %d" % (c.tag, arith)
            out = TB._both(hip_ctx, c.p, arith)
            TB._same(out, what)
            walk = TB._both(hip_ctx, c.p, arith, tscan=0)
            for d in range(2):
                m, st = out[1][d]
                print("%s direction %d: scan tiles bound %d, template %d, walked %d" % (what, d, st["scan_tiles_bound"],
                                                                                       st["scan_tiles_template"], st["scan_tiles_walked"]))
                assert st["used_dense_path"], (what, d, st)
                if RC.RIGS[name]["template"] == "all":
                    assert st["scan_tiles_bound"] > 0 and st["scan_tiles_walked"] == 0, (what, d, st)
                else:
                    assert name in WALKED
                    assert st["scan_tiles_bound"] == 0 and st["scan_tiles_walked"] > 0, (what, d, st)
                for tb in (1, 0):
                    mw, sw = walk[tb][d]
                    assert sw["used_dense_path"] and sw["scan_tiles_template"] == 0, (what, d, sw)
                    SM._assert_bits(mw, m, "%s direction %d: tscan = 0 (tscan_bound = %d)" % (what, d, tb))
                    for key in ("n_eval", "n_pixels", "n_flagged", "n_certified"):
                        assert sw[key] == st[key], (what, d, key, sw[key], st[key])
        if name == "fx_ratio":
            # the strip kernel's chunks hold ranges that slide against x by 0.07 (x - cx): no retry, no fall-back to the
            # per-tile kernel (twoview_wta_run clears used_strip_kernel after a chunk overflow)
            retries = hip_ctx.stats()["band_retries"]                 # (counted since the shared context was made)
            for strip in (4, 8):
                with SM._options(hip_ctx, strip=strip):
                    for d, (ref, oth) in enumerate(DIRECTIONS):
                        hip_ctx.twoview_wta(ref, oth, c.p)
                        st = hip_ctx.stats()
                        assert st["used_dense_path"] and st["used_strip_kernel"] and st["band_retries"] == retries, (c.tag, strip, d, st)
                        SM._assert_bits(hip_ctx.download_depth(ref), out[1][d][0], "%s strip = %d direction %d" % (c.tag, strip, d))


# ---------------------------------------------------------------------------------------------- d. cost rows
ROWS_RIGS = ["moved", "far", "cx_plus", "half_pixel", "fx_ratio"]


@functools.lru_cache(maxsize=None)
def _oracle_rows(name, radius, kind, masks):
    """-> (a memo (h, w, w) of sro_twoview_cost_ncc of (pixel, column of the pixel's row), left to right, NaN until _fill_rows
    is asked for the entry -- the three kernel forms ask for the same ones; the oracle's curve of every pixel)"""
    c = _case(name, radius, kind, masks)
    curves = {(x, y): O.epipolar_curve(c.ocams[0], c.ocams[1], c.imgs[1], c.op, False, x, y) for y in range(c.h) for x in range(c.w)}
    return np.full((c.h, c.w, c.w), np.nan), curves


def _fill_rows(c, table, ys, xs, cxs):
    L = O.lib()
    todo = np.isnan(table[ys, xs, cxs])
    wts, at = None, None
    for y, x, cx in zip(ys[todo], xs[todo], cxs[todo]):
        if at != (x, y):
            wts, at = np.ascontiguousarray(O.weights(c.imgs[0], int(x), int(y), c.op), dtype=np.float64), (x, y)
        table[y, x, cx] = L.sro_twoview_cost_ncc(C.byref(c.imgs[0].c), C.byref(c.imgs[1].c), O.dptr(wts), C.byref(c.op),
                                                 int(x), int(y), int(cx), int(y))
    return table[ys, xs, cxs]


@masked
@kinds
@pytest.mark.parametrize("name", ROWS_RIGS)
def test_cost_rows(hip_ctx, name, radius, kind, masks):
    """the rows in the reference's arithmetic equal the oracle's costs entry by entry, the column being the pixel's returned
    lo + k; the fused rows stay within e0 of them (tests/test_gpu_cert_rows.py); and the returned range of a pixel holds every
    column the oracle's curve of that pixel visits"""
    c = _case(name, radius, kind, masks)
    SM._upload(hip_ctx, c)
    table, curves = _oracle_rows(name, radius, kind, masks)
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
        assert (rng[..., 1] - rng[..., 0] + 1).max() <= exact.shape[2], tag
        n_visited = 0
        for (x, y), cv in curves.items():
            if not c.white[0][y, x] or len(cv) == 0:
                continue
            n_visited += len(cv)
            assert (cv[:, 1] == y).all(), "%s (%d,%d): the oracle leaves the row" % (tag, x, y)
            assert rng[y, x, 0] <= cv[:, 0].min() and cv[:, 0].max() <= rng[y, x, 1], "%s (%d,%d): the oracle visits %d..%d, range %s" % (
                tag, x, y, cv[:, 0].min(), cv[:, 0].max(), rng[y, x])
        assert n_visited > 0, tag
        live = CR._valid(rng, exact.shape[2]) & (exact.view(np.uint64) != CR.UNWRITTEN)
        ys, xs, ks = np.nonzero(live)
        want = _fill_rows(c, table, ys, xs, rng[ys, xs, 0] + ks)
        ok = WO._close(exact[ys, xs, ks], want)
        print("%s: cstride %d, %d live entries against the oracle, %d off; the oracle visits %d columns" % (tag, exact.shape[2], len(ys), (~ok).sum(), n_visited))
        assert len(ys) > 0, tag
        assert ok.all(), "%s: %d of %d entries, first (y, x, k) %s: got %r want %r" % (
            tag, (~ok).sum(), len(ys), [int(a[~ok][0]) for a in (ys, xs, ks)], exact[ys, xs, ks][~ok][0], want[~ok][0])
        worst, n_cert, n_clamp, n_unc = CR._rows_check(hip_ctx, c.p, 0, c.h, strip, tag)
        print("cost rows %s: max |fused - exact| = %.3g e0 over %d certified entries (%d clamps, %d uncertified)" % (tag, worst, n_cert, n_clamp, n_unc))
        assert n_cert > 0, tag


# ---------------------------------------------------------------------------------------------- e. the plan's other consumers
CONSUMER_RIGS = ["moved", "cx_plus"]


@kinds
@pytest.mark.parametrize("name", CONSUMER_RIGS + ["fx_ratio"])
def test_sad_maps_on_both_plans(hip_ctx, name, radius, kind):
    """cost_sad on the dense plan (twoview_strip_sad_kernel) against tests/sad_ref.py, and bit for bit the list plan's maps"""
    SM.check_sad_maps_on_both_plans(hip_ctx, _case(name, radius, kind))


@kinds
@pytest.mark.parametrize("name", CONSUMER_RIGS + ["fx_ratio", "far"])
def test_compute_against_the_oracles_passes_and_cross_check(hip_ctx, name, radius, kind):
    """on `far` the cross-check's geometry cancels coordinates of several hundred against a baseline of 1"""
    c = _case(name, radius, kind)
    SM.check_compute(hip_ctx, c, _oracle(name, radius, kind))
    assert hip_ctx.stats()["used_dense_path"]


@kinds
@pytest.mark.parametrize("name", CONSUMER_RIGS)
def test_subpixel_against_the_cpu_reference(hip_ctx, name, radius, kind):
    c = _case(name, radius, kind)
    figures = SP.compare_with_the_cpu_reference(hip_ctx, c.tag, c.case)
    assert hip_ctx.stats()["used_dense_path"]
    for left_out, counts in figures:
        assert counts[SP.SR.REFINED] > 0, counts


@kinds
@pytest.mark.parametrize("name", CONSUMER_RIGS)
def test_label_costs(hip_ctx, name, radius, kind):
    SM.check_label_costs(hip_ctx, _case(name, radius, kind))


# ---------------------------------------------------------------------------------------------- f. row bands
# (the template pixel is the band's own middle: every band takes another one)
@pytest.mark.parametrize("bands", [None, [(0, 7), (7, 8), (8, 24)]], ids=["rows", "bands"])
@pytest.mark.parametrize("opts", [dict(), dict(strip=8), dict(strip=0)], ids=["defaults", "strip8", "per-tile"])
@kinds
@pytest.mark.parametrize("name", ["moved", "fx_ratio"])
def test_row_bands_give_the_whole_pass(hip_ctx, name, radius, kind, opts, bands):
    c = _case(name, radius, kind)
    SM.check_row_bands_give_the_whole_pass(hip_ctx, c, opts, bands)
    assert hip_ctx.stats()["used_dense_path"]
