"""Every kernel path of the library against the CPU oracle AWAY from the default constants (tests/constants_cases.py: the
table, what each override moves on the oracle and by how much -- tests/test_constants_host.py holds that without a
device).  A kernel that bakes in 50.0, 3, 1e6, 10.0, 1e-10, 120 or 1000, or whose fast path holds near the defaults only,
fails here.

Tolerances are the project's own: 1e-9 relative against the oracle (cases.compare_depth, no pixel left out; the device
exp differs from libm's), bit equality between device paths and between the certified and the reference's arithmetic,
e0 of capi.cert_bound for the fused cost rows, tests/test_gpu_sad.py's for single costs.

Every WTA path keeps the planes of option "wta_outputs" (winner, runner-up and their costs), so none is skipped there:
the first path's planes are held to the oracle's diagnostics by the rule of tests/test_gpu_wta_outputs.py, every other
path's to the first path's bits."""
import ctypes as C
import functools

import numpy as np
import pytest

import cases
import constants_cases as CC
import filter_ref as F
import oracle_ffi as O
import sad_ref as S
import test_gpu_arith_modes as AM
import test_gpu_cert_rows as CR
import test_gpu_small_shapes as SM
import test_gpu_twoview_mrf as TM
import test_gpu_wta_outputs as WO
import twoview_mrf_ref as MR
from stereoreconstruction_amd import capi
from test_gpu_sad import _assert_costs

pytestmark = pytest.mark.gpu

DIRECTIONS = ((0, 1), (1, 0))
_options = SM._options


def _walk(st):
    return not st["used_dense_path"] and not st["used_fused_kernel"]


# every path a rectified pair can take: tests/test_gpu_small_shapes.py's (defaults = arith 3, arith 0, strip 0 / 4 / 8 -- the
# strip kernel's windows come from geodesic_dma_kernel at r = 5 --, tscan 0, fused, the two list orders, geodma 0), the reference's arithmetic in both kernel forms and the curve walk
RECT_PATHS = SM.PATHS + [
    ("arith 0 strip 8", dict(arith=0, strip=8), lambda st: SM._strip(st) and st["n_certified"] == 0),
    ("arith 0 strip 0", dict(arith=0, strip=0), lambda st: WO._dense(st) and not st["used_strip_kernel"] and st["n_certified"] == 0),
    ("curve walk", dict(force_generic=2), _walk),
]
GENERAL_PATHS = WO.GENERAL_PATHS + [("arith 3", dict(arith=3), lambda st: not WO._dense(st)), ("curve walk", dict(force_generic=2), _walk)]
# paths that run fused costs under a certificate when capi.cert_bound(p)["ok"]
CERTIFIED = ("defaults", "strip 0", "strip 4", "strip 8", "tscan 0", "geodma 0 strip 4", "geodma 0 strip 8", "row-run lists", "arith 3")

RECT_ENTRIES = [e for e in CC.ENTRIES if e.case in CC.RECTIFIED and e.witness != "cross"]
GENERAL_ENTRIES = CC.entries(case="geodesic_verged_dist_masks")
MVS_ENTRIES = CC.entries(kind="mvs")
# overrides that reach a cost (the WTA's own constants and the cross-check's do not)
COST_ENTRIES = [e for e in CC.ENTRIES if not e.case.startswith("mvs") and
                not set(dict(e.over)) <= {"second_best_factor", "wta_margin", "inconsistency_thresh"}]
DENSE_COST_ENTRIES = [e for e in COST_ENTRIES if e.case in CC.RECTIFIED]


def _strip_declines(e):
    """the strip kernel's blocked select form drops unusable taps by a multiplication with 0.0 and needs finite weights:
    geodesic windows under geodesic_sigma <= 0 take the per-tile kernel whatever option "strip" says (TvPass, csrc/srh_api.hip)"""
    return CC.build(e)["params"]["weight_kind"] == capi.WEIGHT_GEODESIC and not dict(e.over).get("geodesic_sigma", 50.0) > 0


@functools.lru_cache(maxsize=None)
def _hip(e):
    return cases.hip_inputs(CC.build(e))


def _upload(ctx, e):
    cams, p = _hip(e)
    cases.upload_case(ctx, CC.build(e), cams)
    op = CC.oracle_inputs(e)[2]
    for k, v in e.over:                                       # both sides run under the override
        assert getattr(p, k) == v and getattr(op, k) == v, (k, v)
    return p


def _assert_depth(got, want, tag):
    ok, msg, _ = cases.compare_depth(got, want, 1e-9)
    assert ok, "%s: %s" % (tag, msg)
    return got.size


def _planes_against_the_oracle(e, direction, got, tag):
    """tests/test_gpu_wta_outputs.py's rule: win_xy exact, both costs _close; a pixel may disagree only where a decision of
    the oracle's own scan is within 1e-7 of flipping, and at most 1 % of the WHITE pixels do"""
    ref, oth = DIRECTIONS[direction]
    imgs, ocams, op = CC.oracle_inputs(e)
    diag = CC.oracle_twoview(e, direction)[1]
    white = CC.build(e)["views"][ref][1] == 1
    agree = (got["win_xy"] == diag["win_xy"]).all(axis=2) & WO._close(got["min_cost"], diag["min_cost"]) & \
        WO._close(got["second_cost"], diag["second_cost"])
    bad = np.argwhere(~agree)
    for y, x in bad:
        gap = WO._decision_gap(imgs, ocams, op, ref, oth, int(x), int(y))
        assert gap <= 1e-7, "%s pixel (%d,%d): win %s / %s, min %r / %r, second %r / %r, no decision within 1e-7 of flipping (gap %g)" % (
            tag, x, y, got["win_xy"][y, x], diag["win_xy"][y, x], got["min_cost"][y, x], diag["min_cost"][y, x],
            got["second_cost"][y, x], diag["second_cost"][y, x], gap)
    assert len(bad) <= 0.01 * white.sum(), tag
    assert (got["win_xy"][~white] == -1).all() and np.isposinf(got["min_cost"][~white]).all()
    return len(bad)


def _run_wta_paths(ctx, e, paths):
    p = _upload(ctx, e)
    ok = capi.cert_bound(p)["ok"]
    name = CC.entry_id(e)
    first = None
    compared = 0
    for tag, opts, ran in paths:
        with _options(ctx, wta_outputs=3, **opts):
            res = [WO._pass(ctx, ref, oth, p) for ref, oth in DIRECTIONS]
        for k, (depth, planes, st) in enumerate(res):
            what = "%s [%s] %d>%d" % (name, tag, *DIRECTIONS[k])
            if _strip_declines(e) and opts.get("strip", 0) in (4, 8):
                assert WO._dense(st) and not st["used_strip_kernel"], "%s: the strip kernel ran on weights that are not finite: %s" % (what, st)
            else:
                assert ran(st), "%s: the intended path did not run: %s" % (what, st)
            compared += _assert_depth(depth, CC.oracle_twoview(e, k)[0], what)
            if not ok or opts.get("arith") == 0:
                assert st["n_certified"] == 0, "%s: certified pixels without a certificate: %s" % (what, st)
            elif tag in CERTIFIED:
                assert st["n_certified"] == st["n_pixels"] > 0, "%s: the certified arithmetic did not run: %s" % (what, st)
        if first is None:
            first = res
            off = [_planes_against_the_oracle(e, k, res[k][1], "%s [%s] pass %d" % (name, tag, k)) for k in range(2)]
        else:
            for k in range(2):
                what = "%s [%s] against [%s], pass %d" % (name, tag, paths[0][0], k)
                WO._same_planes(res[k][1], first[k][1], what)
                SM._assert_bits(res[k][0], first[k][0], what + " depth map")
    print("%s: %d paths, %d pixels compared with the oracle's maps, none off; planes: %s pixels on a flipping decision; cert ok %d" % (
        name, len(paths), compared, off, ok))
    return p, ok


# ---------------------------------------------------------------------------------------------- 1. WTA maps, every path
@pytest.mark.parametrize("e", RECT_ENTRIES, ids=CC.entry_id)
def test_rectified_paths_against_the_oracle(hip_ctx, e):
    p, ok = _run_wta_paths(hip_ctx, e, RECT_PATHS)
    # the certified arithmetic against the reference's, bit for bit, in all three kernel forms (both directions)
    for strip in ((0,) if _strip_declines(e) else (0, 4, 8)):
        flagged, certified = AM._assert_certified_equals_exact(hip_ctx, p, strip, "%s strip=%d" % (CC.entry_id(e), strip), must_certify=bool(ok))
        assert ok or certified == 0
        print("  strip=%d: %d pixels certified, %d flagged and redone" % (strip, certified, flagged))
    if e.witness == "branch" or dict(e.over).get("geodesic_sigma", 1.0) < 0 or dict(e.over).get("geodesic_init", 1.0) <= 0:
        assert not CC.sdiv(dict(e.over))                  # the windows kernels' plain division and range-selecting exp ran


@pytest.mark.parametrize("e", GENERAL_ENTRIES, ids=CC.entry_id)
def test_general_geometry_paths_against_the_oracle(hip_ctx, e):
    _run_wta_paths(hip_ctx, e, GENERAL_PATHS)


def test_the_constants_reach_the_device_maps(hip_ctx):
    """the device's own maps move with the constants as the oracle's do (a table entry is a different computation)"""
    d = CC.default_entry("geodesic_rect")
    p = _upload(hip_ctx, d)
    hip_ctx.twoview_wta(0, 1, p)
    base = hip_ctx.download_depth(0)
    _assert_depth(base, CC.oracle_twoview(d, 0)[0], "defaults")
    for e in CC.entries(witness="depth", case="geodesic_rect"):
        hip_ctx.twoview_wta(0, 1, _hip(e)[1])
        share = CC.depth_share(hip_ctx.download_depth(0), base)
        assert abs(share - e.share) <= 0.02, (CC.entry_id(e), share, e.share)


# ---------------------------------------------------------------------------------------------- 2. MultiViewStereo
MVS_PATHS = [("defaults", dict()), ("mvs_staged 0", dict(mvs_staged=0)), ("force_generic 1", dict(force_generic=1))]


@pytest.mark.parametrize("e", MVS_ENTRIES, ids=CC.entry_id)
def test_mvs_paths_against_the_oracle(hip_ctx, e):
    import torch
    p = _upload(hip_ctx, e)
    cams = _hip(e)[0]
    neigh = [list(n) for n in CC.oracle_neighbours(e)]
    assert capi.mvs_neighbours(cams, p) == neigh, CC.entry_id(e)
    if "num_neighbours" in dict(e.over) or "neighbour_min_dot" in dict(e.over):
        assert neigh != [list(n) for n in CC.oracle_neighbours(CC.default_entry(e.case))]
    compared, staged = 0, 0
    for v in range(len(cams)):
        want = CC.oracle_mvs(e, v)[0]
        first = None
        for tag, opts in MVS_PATHS:
            with _options(hip_ctx, **opts):
                hip_ctx.mvs_initial_estimate(v, neigh[v], p)
                got, st = hip_ctx.download_depth(v), hip_ctx.stats()
            what = "%s [%s] view %d" % (CC.entry_id(e), tag, v)
            compared += _assert_depth(got, want, what)
            if tag == "defaults":
                staged += st["mvs_waves_staged"]
                first = (got, st["n_eval"])
            else:
                SM._assert_bits(got, first[0], what + " against the defaults")
                assert st["n_eval"] == first[1], what
            if tag == "mvs_staged 0":
                assert st["mvs_waves_staged"] == 0, (what, st)
    assert staged > 0, "%s: the staged cost kernel took no wave" % CC.entry_id(e)
    # the top-K (cost, depth) lists of view 0, as tests/test_gpu_edge_cases.py holds them to the oracle
    want_d, want_pk, _ = CC.oracle_mvs(e, 0)
    h, w, K = want_pk.shape[:3]
    assert K == p.top_k
    pk = torch.zeros((h, w, K, 2), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    hip_ctx.mvs_initial_estimate(0, neigh[0], p, peaks_dev=pk.data_ptr())
    hip_ctx.synchronize()
    got = pk.cpu().numpy()
    assert np.allclose(got[..., 0], want_pk[..., 0], rtol=0, atol=1e-12), CC.entry_id(e)
    assert np.allclose(got[..., 1], want_pk[..., 1], rtol=1e-9, atol=0), CC.entry_id(e)
    _assert_depth(hip_ctx.download_depth(0), want_d, CC.entry_id(e) + " with peaks")
    pk2 = torch.full((h, w, K, 2), 7.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    with _options(hip_ctx, force_generic=1):
        hip_ctx.mvs_initial_estimate(0, neigh[0], p, peaks_dev=pk2.data_ptr())
        hip_ctx.synchronize()
    assert np.array_equal(got.view(np.uint64), pk2.cpu().numpy().view(np.uint64)), CC.entry_id(e)
    if e.witness == "peaks":
        share = CC.peaks_share(got, CC.oracle_mvs(CC.default_entry(e.case), 0)[1])
        assert share >= CC.MIN_SHARE, (CC.entry_id(e), share)
    print("%s: %d pixels compared over %d views and %d paths, %d peak entries; waves staged %d" % (
        CC.entry_id(e), compared, len(cams), len(MVS_PATHS), got[..., 0].size, staged))


# ---------------------------------------------------------------------------------------------- 3. SAD
@pytest.mark.parametrize("e", CC.SAD_ENTRIES, ids=CC.entry_id)
def test_sad_maps_on_lists_and_on_the_dense_plan(hip_ctx, e):
    p = _upload(hip_ctx, e)
    got = {}
    for sad_dense in (0, 1):
        with _options(hip_ctx, cost=capi.COST_SAD, sad_dense=sad_dense):
            for k, (ref, oth) in enumerate(DIRECTIONS):
                hip_ctx.twoview_wta(ref, oth, p)
                st = hip_ctx.stats()
                what = "%s sad_dense=%d %d>%d" % (CC.entry_id(e), sad_dense, ref, oth)
                assert bool(st["used_dense_path"]) == bool(sad_dense), "%s: %s" % (what, st)
                got[sad_dense, k] = hip_ctx.download_depth(ref)
                SM._assert_bits(got[sad_dense, k], CC.oracle_sad(e, k)[0], what)
    print("%s: %d pixels, both plans, both directions, the restatement's bits" % (CC.entry_id(e), got[0, 0].size))


# ---------------------------------------------------------------------------------------------- 4. cost rows
@functools.lru_cache(maxsize=None)
def _oracle_rows(e):
    """sro_twoview_cost_ncc under the override of every (pixel, column of its row), left to right, on every third row and
    the last: (rows, h x w x w float64 with NaN on the other rows)"""
    imgs, ocams, op = CC.oracle_inputs(e)
    h, w = imgs[0].h, imgs[0].w
    rows = sorted(set(range(0, h, 3)) | {h - 1})
    out = np.full((h, w, w), np.nan)
    L = O.lib()
    for y in rows:
        for x in range(w):
            wts = np.ascontiguousarray(O.weights(imgs[0], x, y, op), dtype=np.float64)
            for cx in range(w):
                out[y, x, cx] = L.sro_twoview_cost_ncc(C.byref(imgs[0].c), C.byref(imgs[1].c), O.dptr(wts), C.byref(op), x, y, cx, y)
    out.setflags(write=False)
    return rows, out


@pytest.mark.parametrize("e", DENSE_COST_ENTRIES, ids=CC.entry_id)
def test_cost_rows_against_the_oracle_and_within_the_bound(hip_ctx, e):
    """form 0 (the reference's arithmetic) entry by entry against sro_twoview_cost_ncc with the oracle's windows under the
    override, in all three kernel forms; then forms 5 and 3 within e0 of form 0 with nothing uncertified after the in-kernel
    redo (tests/test_gpu_cert_rows.py) -- or, where cert_bound(p) says the parameters leave the certificate no ground,
    no fused rows at all"""
    p = _upload(hip_ctx, e)
    name = CC.entry_id(e)
    h = CC.build(e)["views"][0][0].shape[0]
    rows, want_all = _oracle_rows(e)
    cb = capi.cert_bound(p)
    first = None
    for strip in (0, 4, 8):
        tag = "%s strip=%d" % (name, strip)
        with _options(hip_ctx, strip=strip):
            exact, rng, us = hip_ctx.twoview_cost_rows(0, 1, p, 0, h, 0)
        assert us == (strip != 0 and not _strip_declines(e)), tag
        live = CR._valid(rng, exact.shape[2]) & (exact.view(np.uint64) != CR.UNWRITTEN)
        if first is None:
            first = (exact, live)
        else:
            assert np.array_equal(live, first[1]) and np.array_equal(exact.view(np.uint64)[live], first[0].view(np.uint64)[live]), tag + ": not the bits of strip=0"
        sel = np.zeros(live.shape, bool)
        sel[rows] = live[rows]
        ys, xs, ks = np.nonzero(sel)
        want = want_all[ys, xs, rng[ys, xs, 0] + ks]
        assert not np.isnan(want).any()
        ok = WO._close(exact[ys, xs, ks], want)
        assert ok.all(), "%s: %d of %d entries, first (y, x, k) %s: got %r want %r" % (
            tag, (~ok).sum(), len(ys), [int(a[~ok][0]) for a in (ys, xs, ks)], exact[ys, xs, ks][~ok][0], want[~ok][0])
        assert len(ys) > 1000, tag
        line = "cost rows %s: %d entries against the oracle (%d on the clamp, %d bad_ret)" % (
            tag, len(ys), (want == p.max_color_diff).sum(), (want == p.bad_ret).sum())
        if cb["ok"]:
            worst, n_cert, n_clamp, n_unc = CR._rows_check(hip_ctx, p, 0, h, strip, tag)
            print("%s; max |fused - exact| = %.3g e0 over %d certified entries (%d clamps, %d uncertified in the raw form)" % (line, worst, n_cert, n_clamp, n_unc))
        else:
            for form in (5, 3):
                with pytest.raises(capi.StereoHipError) as err:
                    hip_ctx.twoview_cost_rows(0, 1, p, 0, h, form)
                assert err.value.code == capi.SRH_E_UNSUPPORTED
            print("%s; no certificate under these parameters: no fused rows" % line)
    # the override is in the rows: they are not the default constants' rows
    if e.witness == "depth":
        base = _oracle_rows(CC.default_entry(e.case))[1]
        sub = ~np.isnan(want_all)
        assert (want_all[sub] != base[sub]).mean() > 0.02, name


# ---------------------------------------------------------------------------------------------- 5. pair costs, label volume
def _costs_under(got, want, op, tag, **tol):
    _assert_costs(got, want, tag, **tol)
    assert np.array_equal(got == op.bad_ret, want == op.bad_ret), tag + ": bad_ret positions"
    assert np.array_equal(got == op.max_color_diff, want == op.max_color_diff), tag + ": clamp positions"


@pytest.mark.parametrize("e", COST_ENTRIES, ids=CC.entry_id)
def test_pair_costs_against_the_oracle(hip_ctx, e):
    p = _upload(hip_ctx, e)
    imgs, ocams, op = CC.oracle_inputs(e)
    xy = CC.pairs(e)
    for ref, oth in DIRECTIONS:
        tag = "%s %d>%d" % (CC.entry_id(e), ref, oth)
        ncc = hip_ctx.twoview_pair_costs(ref, oth, p, xy, capi.COST_NCC)
        want = S.pair_costs_ncc(imgs[ref], imgs[oth], op, xy)
        _costs_under(ncc, want, op, tag + " ncc", rtol=1e-9)
        sad = hip_ctx.twoview_pair_costs(ref, oth, p, xy, capi.COST_SAD)
        want_sad = S.pair_costs_sad(imgs[ref], imgs[oth], op, xy)
        _assert_costs(sad, want_sad, tag + " sad")
        assert np.array_equal(sad == op.bad_ret, want_sad == op.bad_ret), tag + " sad: bad_ret positions"
        print("%s: %d pairs; ncc: %d bad_ret, %d on the clamp; sad: %d bad_ret" % (
            tag, len(xy), (want == op.bad_ret).sum(), (want == op.max_color_diff).sum(), (want_sad == op.bad_ret).sum()))
    if "bad_ret" in dict(e.over):
        assert (want == op.bad_ret).any() and (want_sad == op.bad_ret).any(), CC.entry_id(e)


@pytest.mark.parametrize("e", CC.entries(case=("geodesic_masks", "adaptive_masks"), has=("bad_ret",)), ids=CC.entry_id)
def test_label_costs_under_another_fill_and_cutoff(hip_ctx, e):
    """the loop of tests/test_gpu_twoview_mrf.py::test_label_costs with bad_ret and weight_cutoff overridden"""
    p = _upload(hip_ctx, e)
    case = CC.build(e)
    imgs, ocams, op = CC.oracle_inputs(e)
    fill = MR.fill_value(p.window_radius, p.bad_ret)
    assert fill != MR.fill_value(p.window_radius, 1000.0) and p.bad_ret == 0.02
    rng = np.random.default_rng(len(CC.entry_id(e)))
    for ref, oth in DIRECTIONS:
        want_pix = TM._cpu_label_pixels(case, ocams, op, ref, oth)
        has = want_pix[..., 0] != TM.NONE
        assert has.any() and (~has).any()
        yy, xx, dd = np.nonzero(has)
        xy = np.stack([xx, yy, want_pix[yy, xx, dd, 0], want_pix[yy, xx, dd, 1]], 1).astype(np.int32)
        sub = rng.choice(len(xy), size=min(600, len(xy)), replace=False)
        for kind, kname in ((capi.COST_NCC, "ncc"), (capi.COST_SAD, "sad")):
            tag = "%s %s %d>%d" % (CC.entry_id(e), kname, ref, oth)
            with _options(hip_ctx, cost=kind):
                cost, pix = hip_ctx.twoview_label_costs(ref, oth, p)
            assert np.array_equal(pix, want_pix), "%s: %d label pixels differ" % (tag, (pix != want_pix).any(axis=-1).sum())
            assert (cost[~has] == fill).all(), tag
            pc = hip_ctx.twoview_pair_costs(ref, oth, p, xy, kind)
            SM._assert_bits(cost[yy, xx, dd], pc, tag + " vs pair costs")
            if kind == capi.COST_SAD:
                _assert_costs(pc[sub], S.pair_costs_sad(imgs[ref], imgs[oth], op, xy[sub]), tag + " oracle")
            else:
                _costs_under(pc[sub], S.pair_costs_ncc(imgs[ref], imgs[oth], op, xy[sub]), op, tag + " oracle", rtol=1e-9)
            assert (pc == op.bad_ret).any(), tag


# ---------------------------------------------------------------------------------------------- 6. cross-checks
@pytest.mark.parametrize("e", CC.entries(witness="cross"), ids=CC.entry_id)
def test_twoview_compute_under_another_inconsistency_threshold(hip_ctx, e):
    p = _upload(hip_ctx, e)
    want = CC.oracle_cross(e)
    base = CC.oracle_cross(CC.default_entry(e.case))
    for overlap in (1, 0):
        with _options(hip_ctx, tv_overlap=overlap):
            got = hip_ctx.twoview_compute(0, 1, p)
        for k in range(2):
            _assert_depth(got[k], want[k], "%s tv_overlap=%d map %d" % (CC.entry_id(e), overlap, k))
    # the cross-check alone, from the oracle's WTA maps
    for k in range(2):
        hip_ctx.upload_depth(k, np.array(CC.oracle_twoview(e, k)[0]))
    hip_ctx.twoview_cross_check(0, 1, p)
    for k in range(2):
        _assert_depth(hip_ctx.download_depth(k), want[k], "%s cross-check alone, map %d" % (CC.entry_id(e), k))
    share = float(np.mean([(CC.class_of(g) != CC.class_of(b)).mean() for g, b in zip(got, base)]))
    print("%s: %d pixels compared per map; %.3f change class against the default threshold" % (CC.entry_id(e), got[0].size, share))
    assert share >= CC.MIN_SHARE


@pytest.mark.parametrize("factor", [0.5, 2.0], ids=["half", "twice"])
def test_mvs_cross_check_under_another_threshold(hip_ctx, factor):
    d = CC.default_entry("mvs_geodesic")
    case = CC.build(d)
    case = dict(case, params=dict(case["params"], cross_check_threshold=factor * case["params"]["cross_check_threshold"]))
    imgs, ocams, op = cases.oracle_inputs(case)
    cams, p = cases.hip_inputs(case)
    assert p.cross_check_threshold == op.cross_check_threshold == factor * CC.oracle_inputs(d)[2].cross_check_threshold
    cases.upload_case(hip_ctx, case, cams)
    nv = len(cams)
    start = [np.array(CC.oracle_mvs(d, v)[0]) for v in range(nv)]
    ref = [s.copy() for s in start]
    base = [s.copy() for s in start]
    for v in range(nv):
        O.mvs_cross_check(imgs, ocams, v, op, ref)
        O.mvs_cross_check(*CC.oracle_inputs(d)[:2], v, CC.oracle_inputs(d)[2], base)
    for v in range(nv):
        hip_ctx.upload_depth(v, start[v])
    for v in range(nv):
        hip_ctx.mvs_cross_check(list(range(nv)), v, p)
    for v in range(nv):
        _assert_depth(hip_ctx.download_depth(v), ref[v], "cross_check_threshold x %g, view %d" % (factor, v))
    moved = sum(int((CC.class_of(r) != CC.class_of(b)).sum()) for r, b in zip(ref, base))
    print("cross_check_threshold x %g: %d pixels change class against the case's own threshold" % (factor, moved))
    assert moved > 0


# ---------------------------------------------------------------------------------------------- 7. hole filling
FILTER_ENTRIES = [CC._e("geodesic_rect", "depth", 0.717, geodesic_sigma=7.3), CC._e("geodesic_rect", "depth", 0.123, geodesic_iters=1),
                  CC._e("adaptive_rect", "depth", 0.607, adaptive_color_sigma=2.5)]


@pytest.mark.parametrize("e", FILTER_ENTRIES, ids=CC.entry_id)
def test_weighted_median_under_other_window_constants(hip_ctx, e):
    """constants for which exp(-geodesic_init/geodesic_sigma) <= 1e-10 still holds: the device's skip of the taps outside
    the image is the reference's result, against tests/filter_ref.py"""
    assert e in CC.ENTRIES and CC.median_premise(dict(e.over))
    p = _upload(hip_ctx, e)
    case = CC.build(e)
    default_p = _hip(CC.default_entry(e.case))[1]
    differs = 0
    for slot in (0, 1):
        rgba, mask = case["views"][slot][0], case["views"][slot][1]
        depth = np.array(CC.oracle_cross(e)[slot])
        assert (~np.isfinite(depth) & (mask == 1 if mask is not None else True)).sum() > 50
        for flags in (capi.FILTER_MEDIAN, capi.FILTER_GAPS | capi.FILTER_MEDIAN):
            hip_ctx.upload_depth(slot, depth)
            info = hip_ctx.filter_invalid(slot, p, flags)
            got = hip_ctx.download_depth(slot)
            want = F.filter_map(rgba, mask, depth, F.oparams(p), flags)
            assert F.same_bits(got, want), "%s slot %d flags %d: %d pixels differ" % (
                CC.entry_id(e), slot, flags, (got.view(np.uint64) != want.view(np.uint64)).sum())
            assert info["median_filled"] > 0
            differs += int((want.view(np.uint64) != F.filter_map(rgba, mask, depth, F.oparams(default_p), flags).view(np.uint64)).sum())
    print("%s: %d filled values are not the default constants'" % (CC.entry_id(e), differs))
    assert differs > 0


@pytest.mark.parametrize("over", [dict(geodesic_init=30.0), dict(geodesic_sigma=-50.0), dict(geodesic_init=-100.0)], ids=str)
def test_weighted_median_outside_its_premise_is_refused(hip_ctx, over):
    """exp(-geodesic_init/geodesic_sigma) > 1e-10 (0.55 at geodesic_init 30): the reference keeps taps outside the image,
    the device would skip them -- SRH_E_UNSUPPORTED before anything is launched, from srh_twoview_compute too"""
    assert not CC.median_premise(over)
    e = CC._e("geodesic_rect", "depth", 0.0, **over)
    p = _upload(hip_ctx, e)
    depth = np.array(CC.oracle_cross(CC.default_entry("geodesic_rect"))[0])
    hip_ctx.upload_depth(0, depth)
    for flags in (capi.FILTER_MEDIAN, capi.FILTER_GAPS | capi.FILTER_MEDIAN):
        with pytest.raises(capi.StereoHipError) as err:
            hip_ctx.filter_invalid(0, p, flags)
        assert err.value.code == capi.SRH_E_UNSUPPORTED
        assert F.same_bits(hip_ctx.download_depth(0), depth)                      # nothing ran
    # the gap fill reads no window: served as before
    hip_ctx.filter_invalid(0, p, capi.FILTER_GAPS)
    assert F.same_bits(hip_ctx.download_depth(0), F.filter_map(CC.build(e)["views"][0][0], CC.build(e)["views"][0][1], depth, F.oparams(p), capi.FILTER_GAPS))
    # adaptive windows are 0 outside the image whatever the constants
    pa = capi.params_twoview(**dict(CC.build(e)["params"], weight_kind=capi.WEIGHT_ADAPTIVE))
    hip_ctx.upload_depth(0, depth)
    hip_ctx.filter_invalid(0, pa, capi.FILTER_MEDIAN)
    # srh_twoview_compute with the option: refused before the first progress step, the slot's map untouched
    hip_ctx.upload_depth(0, depth)
    steps = []
    hip_ctx.set_hooks(progress=lambda s, stage: steps.append(s))
    hip_ctx.set_option("filter_invalid", capi.FILTER_MEDIAN)
    try:
        with pytest.raises(capi.StereoHipError) as err:
            hip_ctx.twoview_compute(0, 1, p)
    finally:
        hip_ctx.set_option("filter_invalid", 0)
        hip_ctx.set_hooks()
    assert err.value.code == capi.SRH_E_UNSUPPORTED and steps == []
    assert F.same_bits(hip_ctx.download_depth(0), depth)


# ---------------------------------------------------------------------------------------------- 8. weights above 1
@pytest.mark.parametrize("e", CC.entries(has=("geodesic_init",), case=CC.RECTIFIED), ids=CC.entry_id)
def test_a_negative_start_value_keeps_the_certificate(hip_ctx, e):
    """geodesic_init < 0 gives window weights up to wmax = exp(-geodesic_init/geodesic_sigma) > 1: cert_bound widens G, k1 and
    k2 by wmax (srh_wta.hpp, tests/test_cert_bound.py) and the certified arithmetic runs, within e0 of the reference's rows
    and with its bits in the maps (test_cost_rows_..., test_rectified_paths_... above, on the same entries).  Measured with
    the unscaled constants as well: max |fused - exact| = 4e-5 e0 at geodesic_init = -100 -- the scaling is the derivation's
    due, not an observed failure."""
    p = _upload(hip_ctx, e)
    cb = capi.cert_bound(p)
    base = capi.cert_bound(_hip(CC.default_entry(e.case))[1])
    wmax = np.exp(-p.geodesic_init / p.geodesic_sigma) if p.geodesic_init < 0 else 1.0
    assert cb["ok"] == 1 and cb["e0"] == base["e0"] and abs(cb["k1"] / base["k1"] - wmax) < 1e-12 * wmax, CC.entry_id(e)
    h = CC.build(e)["views"][0][0].shape[0]
    for strip in (0, 8):
        with _options(hip_ctx, strip=strip):
            hip_ctx.twoview_wta(0, 1, p)
            st = hip_ctx.stats()
        assert st["n_certified"] == st["n_pixels"] > 0, (CC.entry_id(e), strip, st)
        _assert_depth(hip_ctx.download_depth(0), CC.oracle_twoview(e, 0)[0], "%s strip=%d" % (CC.entry_id(e), strip))
        worst, n_cert, n_clamp, n_unc = CR._rows_check(hip_ctx, p, 0, h, strip, "%s strip=%d" % (CC.entry_id(e), strip))
        print("%s strip=%d: wmax %.3g, max |fused - exact| = %.3g e0 over %d certified entries, %d uncertified in the raw form" % (
            CC.entry_id(e), strip, wmax, worst, n_cert, n_unc))
        assert n_cert > 0
