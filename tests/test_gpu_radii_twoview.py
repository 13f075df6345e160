"""TwoViewStereo at the window radii the rest of the suite leaves out.  check_params accepts 1 .. 15 and the pass driver
(twoview_wta_run, csrc/srh_api.hip) changes kernels with the radius:

  r = 1, 3, 4   no dense plan (TvPass::plan: r = 5 and 2 only); the candidate lists in row runs (srh_rows.hip:
                twoview_rows_cost_kernel<R, 0|3|5>, twoview_rows_refill_kernel<R>), in list order (srh_list.hip:
                twoview_list_cost_kernel<R>), the SAD row kernels (srh_sad.hip) -- each instantiation sizes its LDS and its
                window layout by R -- and the walk kernel under force_generic = 2;
  r = 6 .. 15   no lists either: weights_kernel, then twoview_generic_kernel with windows of up to 31 x 31 = 961 taps, the
                band sized at that T; twoview_winner_costs_kernel and the sub-pixel kernels take R at run time; pair costs,
                label costs (hence the MRF and SGM stages) and the weighted median refuse r > 5.

Sections b and c below hold every one of these to the CPU oracle.  Every tolerance is the one the named existing test
uses: cases.compare_depth at 1e-9 against the oracle, bit equality between device paths and against tests/sad_ref.py, the
decision-gap rule of tests/test_gpu_wta_outputs.py for the by-products, test_against_the_cpu_reference's for option
"subpixel".  tests/test_gpu_arith_modes.py states what arith 1 and 2 must satisfy on the dense plan only; it says nothing
of the list paths, so nothing is asserted of them here."""
import numpy as np
import pytest

import cases
import filter_ref as F
import oracle_ffi as O
import sad_ref as S
import subpixel_ref as SR
import test_gpu_filter as TF
import test_gpu_sad as GS
import test_gpu_small_shapes as SM
import test_gpu_subpixel as SP
import test_gpu_twoview_mrf as TM
import test_gpu_twoview_sgm as TS
import test_gpu_wta_outputs as WO
from stereoreconstruction_amd import capi

pytestmark = pytest.mark.gpu

DIRECTIONS = SM.DIRECTIONS
KINDS = ((1, "geodesic"), (0, "adaptive"))
LIST_RADII = (1, 3, 4)
WALK_RADII = (6, 9, 15)
MAIN = (44, 26, 10)


def _id(shape, radius, kind, masks=False, general=False):
    return "%s-r%d-%s%s%s" % (SM.SS.shape_id(shape), radius, dict(KINDS)[kind], "-masks" if masks else "", "-verged-distorted" if general else "")


def _cases(radii, shapes, variants=((False, False),), extra=()):
    """(shape, radius, kind, masks, general): every shape plain, the main shape in every variant as well"""
    out = []
    for r in radii:
        todo = [(s, False, False) for s in shapes] + [(MAIN, m, g) for m, g in variants if m or g] + [(s, False, False) for s, rr in extra if rr == r]
        out += [(s, r, k, m, g) for s, m, g in todo for k, _ in KINDS]
    return out


def _params(table):
    return pytest.mark.parametrize("shape,radius,kind,masks,general", table, ids=[_id(*c) for c in table])


# 33x7x12: one column past the 32-pixel window tile, the 8-pixel cost tiles ragged; 8x5x6 at r = 4: w <= 2r
B_SHAPES = [MAIN, (33, 7, 12), (31, 9, 8), (48, 1, 8), (1, 9, 4)]
B_CASES = _cases(LIST_RADII, B_SHAPES, variants=((True, False), (True, True)), extra=[((8, 5, 6), 4)])
# (name, options, the cost kernel that has to run, the one that must not: names of Context.profile())
ROWS_NCC, LIST_NCC = "twoview_rows_cost_kernel", "twoview_list_cost_kernel"
ROWS_SAD, LIST_SAD = "twoview_rows_sad_kernel", "twoview_list_sad_kernel"
WALK = "twoview_generic_kernel"
LIST_PATHS = [
    ("row-run lists arith 0", dict(force_generic=1, list_rows=1, arith=0), ROWS_NCC, LIST_NCC),
    ("row-run lists arith 3", dict(force_generic=1, list_rows=1, arith=3), ROWS_NCC, LIST_NCC),
    ("list order arith 0", dict(force_generic=1, list_rows=0, arith=0), LIST_NCC, ROWS_NCC),
    ("list order", dict(force_generic=1, list_rows=0), LIST_NCC, ROWS_NCC),
    ("defaults", dict(), ROWS_NCC, LIST_NCC),
]


def _lists(st):
    return st["used_dense_path"] == 0 and st["used_fused_kernel"] == 0


def _depth_pass(ctx, ref, oth, p):
    ctx.twoview_wta(ref, oth, p)
    return ctx.download_depth(ref), None, ctx.stats()


def _fresh_pass(ctx, c, ref, oth, ran, ran_not, what, run=WO._pass):
    """One WTA pass on freshly uploaded views (the caller set the options) -> (depth map, planes, stats), with the cost
    kernels it launched checked by name.  The upload is what makes option list_rows = 1 mean row runs: a standing row-run pass
    teaches the context how the pair's lists are best evaluated (tv_learn_lists, csrc/srh_api.hip: more than 2.2 cost slots
    per candidate -- short spans, as on a view narrower than the 8-column blocks -- and the pair's later passes go in list
    order, which has no certified form), and an upload forgets it."""
    SM._upload(ctx, c)
    ctx.profile_reset()
    ctx.profile_enable(True)
    try:
        out = run(ctx, ref, oth, c.p)
    finally:
        ctx.synchronize()
        ctx.profile_enable(False)
    launched = set(ctx.profile().keys())
    assert ran in launched and ran_not not in launched and _lists(out[2]), "%s: the intended path did not run: %s, %s" % (
        what, sorted(k for k in launched if k.startswith("twoview")), out[2])
    return out


# ================================================================================================ b. r = 1, 3, 4
@_params(B_CASES)
def test_every_list_path_gives_the_walk_kernels_bits(hip_ctx, shape, radius, kind, masks, general):
    """the walk kernel in the reference's arithmetic against the oracle, then every list path against the walk kernel bit for
    bit: depth map, winners, runners-up and both costs (test_dense_path_matches_oracle_and_generic's scheme at r = 2, 5)"""
    c = SM._case(shape, radius, kind, masks, general)
    want = SM._oracle(shape, radius, kind, masks, general)
    SM._upload(hip_ctx, c)
    walk = WO._yardstick(hip_ctx, c.p)
    for k, (ref, oth) in enumerate(DIRECTIONS):
        d, _, st = walk[k]
        depth, diag = want[k]
        print("%s walk %d>%d: finite %d, +INF %d, NaN %d, n_eval %d / %d" % (c.tag, ref, oth, np.isfinite(d).sum(), np.isposinf(d).sum(),
                                                                             np.isnan(d).sum(), st["n_eval"], diag["n_eval"]))
        SM._assert_depth(d, depth, "%s walk kernel %d>%d" % (c.tag, ref, oth))
        assert st["n_eval"] == diag["n_eval"] and _lists(st), (c.tag, st)
        assert st["n_pixels"] == int(c.white[ref].sum())
    for tag, opts, ran, ran_not in LIST_PATHS:
        with SM._options(hip_ctx, wta_outputs=3, **opts):
            for k, (ref, oth) in enumerate(DIRECTIONS):
                what = "%s %s %d>%d" % (c.tag, tag, ref, oth)
                d, got, st = _fresh_pass(hip_ctx, c, ref, oth, ran, ran_not, what)
                WO._same_planes(got, walk[k][1], what)
                SM._assert_bits(d, walk[k][0], what + " depth map")
                assert st["n_pixels"] == walk[k][2]["n_pixels"], what
                if opts.get("arith") == 0:
                    assert st["n_certified"] == 0, what
                elif opts.get("list_rows", 1):
                    # the certified arithmetic is the row runs' (list order has the reference's only): the whole pass is
                    # scanned under it, flagged pixels redone
                    print("%s: certified %d, flagged %d of %d pixels" % (what, st["n_certified"], st["n_flagged"], st["n_pixels"]))
                    assert st["n_certified"] == st["n_pixels"] and 0 <= st["n_flagged"] <= st["n_pixels"], (what, st)
                    assert st["n_certified"] + st["n_flagged"] >= st["n_pixels"], (what, st)
    if shape[0] > 1 and shape[1] > 1:
        assert any(np.isfinite(w[0]).any() for w in walk), c.tag


BAND_PATHS = [("row-run lists", dict(), ROWS_NCC, LIST_NCC), ("list order", dict(list_rows=0), LIST_NCC, ROWS_NCC),
              ("walk", dict(force_generic=2), WALK, ROWS_NCC)]


@pytest.mark.parametrize("kind", [k for k, _ in KINDS], ids=[n for _, n in KINDS])
@pytest.mark.parametrize("radius", LIST_RADII)
def test_bands_give_the_bits_of_one_band(hip_ctx, radius, kind):
    """44x96x10 under band_budget_mb = 1.  A band holds at least its windows, T * 8 * 44 bytes a row: 28512 B at r = 4 (at most
    36 rows, 3 bands), 17248 B at r = 3 (60 rows, 2 bands); at r = 1 (3168 B) the windows alone would fit, and it is the lists'
    cost slots and candidates that the budget divides."""
    shape = (44, 96, 10)
    c = SM._case(shape, radius, kind)
    for tag, opts, ran, ran_not in BAND_PATHS:
        for ref, oth in DIRECTIONS:
            what = "%s %s banded %d>%d" % (c.tag, tag, ref, oth)
            with SM._options(hip_ctx, wta_outputs=3, **opts):
                d1, one, st = _fresh_pass(hip_ctx, c, ref, oth, ran, ran_not, what)
            with SM._options(hip_ctx, wta_outputs=3, band_budget_mb=1, **opts):
                dn, many, stn = _fresh_pass(hip_ctx, c, ref, oth, ran, ran_not, what)
            assert stn["band_budget_bytes"] == 1 << 20, what
            assert stn["n_eval"] == st["n_eval"] and stn["n_pixels"] == st["n_pixels"], what
            WO._same_planes(many, one, what)
            SM._assert_bits(dn, d1, what)
            assert np.isfinite(d1).any()


@pytest.mark.parametrize("opts", [dict(), dict(list_rows=0), dict(force_generic=2)], ids=["row-runs", "list-order", "walk"])
@pytest.mark.parametrize("kind", [k for k, _ in KINDS], ids=[n for _, n in KINDS])
@pytest.mark.parametrize("radius", LIST_RADII)
@pytest.mark.parametrize("shape", [(33, 7, 12), (31, 9, 8)], ids=SM.SS.shape_id)
def test_rows_one_at_a_time_give_the_whole_pass(hip_ctx, shape, radius, kind, opts):
    SM.test_rows_one_at_a_time_give_the_whole_pass(hip_ctx, shape, radius, kind, opts)


SAD_KERNELS = dict(rows=(ROWS_SAD, LIST_SAD), list_order=(LIST_SAD, ROWS_SAD), walk=(WALK, ROWS_SAD))


@_params(B_CASES)
def test_sad_on_every_general_path(hip_ctx, shape, radius, kind, masks, general):
    """cost = SAD on the PATHS of tests/test_gpu_sad.py against tests/sad_ref.py: bit for bit, NaN and INF positions included"""
    c = SM._case(shape, radius, kind, masks, general)
    want = [S.twoview_wta_sad(c.imgs[r], c.imgs[o], c.ocams[r], c.ocams[o], c.op) for r, o in DIRECTIONS]
    assert [tag for tag, _ in GS.PATHS] == list(SAD_KERNELS)
    for tag, opts in GS.PATHS:
        with SM._options(hip_ctx, cost=capi.COST_SAD, **opts):
            for k, (ref, oth) in enumerate(DIRECTIONS):
                what = "%s sad %s %d>%d" % (c.tag, tag, ref, oth)
                d, _, st = _fresh_pass(hip_ctx, c, ref, oth, *SAD_KERNELS[tag], what, run=_depth_pass)
                SM._assert_bits(d, want[k], what)


def _planes_against_the_oracle(ctx, c, want, ran, ran_not):
    """the planes of both directions under the default options, held to the oracle's diagnostics; yields them"""
    excused = 0
    for k, (ref, oth) in enumerate(DIRECTIONS):
        with SM._options(ctx, wta_outputs=3):
            _, got, st = _fresh_pass(ctx, c, ref, oth, ran, ran_not, "%s %d>%d" % (c.tag, ref, oth))
        excused += WO.compare_planes_with_the_oracle(got, want[k][1], c.white[ref], c.imgs, c.ocams, c.op, ref, oth, c.tag)
        assert np.isfinite(got["min_cost"][got["win_xy"][..., 0] >= 0]).all()
        assert np.isfinite(got["second_cost"][got["runner_xy"][..., 0] >= 0]).all()
        assert np.isposinf(got["min_cost"][c.white[ref] & (got["win_xy"][..., 0] < 0)]).all()
        yield ref, oth, got
    print("%s: %d pixels excused by the decision-gap rule" % (c.tag, excused))


@_params(B_CASES)
def test_by_products_against_the_oracle_and_the_pair_costs(hip_ctx, shape, radius, kind, masks, general):
    c = SM._case(shape, radius, kind, masks, general)
    want = SM._oracle(shape, radius, kind, masks, general)
    for ref, oth, got in _planes_against_the_oracle(hip_ctx, c, want, ROWS_NCC, LIST_NCC):
        # (a one-row or one-column view has winners but no runner-up: nothing for the pair costs of second_cost to be)
        if shape[0] > 1 and shape[1] > 1:
            WO._assert_pair_costs(hip_ctx, ref, oth, c.p, got, capi.COST_NCC, "%s %d>%d" % (c.tag, ref, oth))


@pytest.mark.parametrize("kind", [k for k, _ in KINDS], ids=[n for _, n in KINDS])
@pytest.mark.parametrize("radius", LIST_RADII)
def test_label_costs(hip_ctx, radius, kind):
    SM.test_label_costs(hip_ctx, (33, 7, 12), radius, kind)


def test_compute_sgm_at_radius_3(hip_ctx):
    """srh_twoview_compute_sgm = label costs -> tests/sgm_ref.py -> the oracle's cross-check (test_compute_sgm_end_to_end)"""
    c = SM._case(MAIN, 3, 1)
    SM._upload(hip_ctx, c)
    dl, dr, maps, vols = TS._chain(hip_ctx, c.case, c.ocams, c.op, c.p)
    gl, gr, infos = hip_ctx.twoview_compute_sgm(0, 1, c.p)
    labels, D, sums = hip_ctx.twoview_sgm_state(*hip_ctx.twoview_sgm_dims(), want_costs=True)
    SM._assert_bits(gl, dl, c.tag + " left")
    SM._assert_bits(gr, dr, c.tag + " right")
    for k in range(2):
        assert infos[k]["paths"] == 8
        assert abs(infos[k]["energy"] - maps[k]["energy"]) <= 1e-10 * max(1.0, abs(maps[k]["energy"]))
    assert np.array_equal(labels, maps[1]["labels"]) and S.same_bits(sums, maps[1]["S"]) and S.same_bits(D, vols[1])
    assert np.isfinite(gl).any()


def test_compute_mrf_at_radius_3(hip_ctx):
    """srh_twoview_compute_mrf = label costs -> tests/twoview_mrf_ref.py -> the oracle's cross-check (test_compute_mrf_end_to_end)"""
    c = SM._case(MAIN, 3, 0, True)
    SM._upload(hip_ctx, c)
    dl, dr, maps = TM._chain(hip_ctx, c.case, c.imgs, c.ocams, c.op, c.p, {})
    gl, gr, infos = hip_ctx.twoview_compute_mrf(0, 1, c.p)
    labels, D, M = hip_ctx.twoview_mrf_state(*hip_ctx.twoview_mrf_dims(), want_costs=True)
    SM._assert_bits(gl, dl, c.tag + " left")
    SM._assert_bits(gr, dr, c.tag + " right")
    for k in range(2):
        assert infos[k]["iterations"] == maps[k]["iterations"]
        assert abs(infos[k]["energy_final"] - maps[k]["energy_final"]) <= 1e-10 * max(1.0, abs(maps[k]["energy_final"]))
    assert np.array_equal(labels, maps[1]["labels"]) and not (M != maps[1]["messages"]).any()
    mask = c.case["views"][0][1]
    assert np.isnan(gl[mask != 1]).all() and (~np.isnan(gl[mask == 1])).all()


@pytest.mark.parametrize("kind", [k for k, _ in KINDS], ids=[n for _, n in KINDS])
@pytest.mark.parametrize("radius", LIST_RADII)
def test_filter_invalid(hip_ctx, radius, kind):
    """the weighted median builds its window in LDS per lane, sized by r: whole maps against tests/filter_ref.py"""
    w, h = 90, 70
    rgba, mask, depth = TF._synthetic(w, h, 0x5EED0F40 + radius + kind)
    hip_ctx.upload_view(0, rgba, mask, TF._cam(w, h))
    got, info = TF._check(hip_ctx, 0, rgba, mask, depth, TF._params(radius, kind), capi.FILTER_GAPS | capi.FILTER_MEDIAN,
                          tag="90x70 r%d k%d" % (radius, kind))
    assert info["holes"] > 0 and info["gap_filled"] > 0 and info["median_filled"] > 0
    TF._check(hip_ctx, 0, rgba, mask, depth, TF._params(radius, kind), capi.FILTER_MEDIAN, tag="90x70 r%d k%d median" % (radius, kind))


# ================================================================================================ c. r = 6, 9, 15
# 20x12x8: smaller than the window in both directions at r = 15; 33x1x8: one row
C_SHAPES = [MAIN, (20, 12, 8), (33, 1, 8)]
C_CASES = [(s, r, k, m, False) for r in WALK_RADII for s in C_SHAPES for k, _ in KINDS for m in (False, True)]
C_PLANES = [c for c in C_CASES if c[1] in (6, 15)]


@_params(C_CASES)
def test_large_windows_whole_maps(hip_ctx, shape, radius, kind, masks, general):
    """weights_kernel, then twoview_generic_kernel with (2r + 1)^2 taps a window, under the default options: NCC against the
    oracle, SAD against tests/sad_ref.py bit for bit; the oracle's count of evaluations under both"""
    c = SM._case(shape, radius, kind, masks)
    want = SM._oracle(shape, radius, kind, masks)
    SM._upload(hip_ctx, c)
    hip_ctx.profile_reset()
    hip_ctx.profile_enable(True)
    try:
        for k, (ref, oth) in enumerate(DIRECTIONS):
            hip_ctx.twoview_wta(ref, oth, c.p)
            got, st = hip_ctx.download_depth(ref), hip_ctx.stats()
            depth, diag = want[k]
            what = "%s %d>%d" % (c.tag, ref, oth)
            print("%s: finite %d, +INF %d, NaN %d, n_eval %d / %d" % (what, np.isfinite(got).sum(), np.isposinf(got).sum(), np.isnan(got).sum(),
                                                                     st["n_eval"], diag["n_eval"]))
            SM._assert_depth(got, depth, what)
            assert st["n_eval"] == diag["n_eval"] and _lists(st) and st["n_certified"] == 0, (what, st)
            assert st["n_pixels"] == int(c.white[ref].sum()), what
    finally:
        hip_ctx.synchronize()
        hip_ctx.profile_enable(False)
    launched = set(hip_ctx.profile().keys())
    assert "twoview_generic_kernel" in launched, sorted(launched)
    sad = [S.twoview_wta_sad(c.imgs[r], c.imgs[o], c.ocams[r], c.ocams[o], c.op) for r, o in DIRECTIONS]
    with SM._options(hip_ctx, cost=capi.COST_SAD):
        for k, (ref, oth) in enumerate(DIRECTIONS):
            hip_ctx.twoview_wta(ref, oth, c.p)
            st = hip_ctx.stats()
            SM._assert_bits(hip_ctx.download_depth(ref), sad[k], "%s sad %d>%d" % (c.tag, ref, oth))
            assert st["n_eval"] == want[k][1]["n_eval"] and _lists(st), (c.tag, st)
    if shape[1] > 1:
        assert any(np.isfinite(w[0]).any() for w in want), c.tag


@pytest.mark.parametrize("masks", [False, True], ids=["plain", "masks"])
@pytest.mark.parametrize("kind", [k for k, _ in KINDS], ids=[n for _, n in KINDS])
def test_large_windows_in_bands(hip_ctx, kind, masks):
    """r = 15: 961 taps * 8 B * 44 pixels = 338272 B of windows a row, so band_rows (csrc/srh_api.hip) gives 1 MB three rows and
    the 26 rows go in 9 bands"""
    c = SM._case(MAIN, 15, kind, masks)
    assert (1 << 20) // (961 * 8 * 44) == 3
    SM._upload(hip_ctx, c)
    for cost in (capi.COST_NCC, capi.COST_SAD):
        for ref, oth in DIRECTIONS:
            with SM._options(hip_ctx, wta_outputs=3, cost=cost):
                d1, one, st = WO._pass(hip_ctx, ref, oth, c.p)
            with SM._options(hip_ctx, wta_outputs=3, cost=cost, band_budget_mb=1):
                dn, many, stn = WO._pass(hip_ctx, ref, oth, c.p)
            what = "%s cost %d banded %d>%d" % (c.tag, cost, ref, oth)
            assert stn["band_budget_bytes"] == 1 << 20 and st["band_budget_bytes"] >= 961 * 8 * 44 * 26, what
            assert stn["n_eval"] == st["n_eval"], what
            WO._same_planes(many, one, what)
            SM._assert_bits(dn, d1, what)


@pytest.mark.parametrize("masks", [False, True], ids=["plain", "masks"])
@pytest.mark.parametrize("kind", [k for k, _ in KINDS], ids=[n for _, n in KINDS])
def test_compute_at_radius_9(hip_ctx, kind, masks):
    """srh_twoview_compute = the oracle's two passes + its cross-check, with the second pass beside the first or after it"""
    c = SM._case(MAIN, 9, kind, masks)
    (dl, _), (dr, _) = SM._oracle(MAIN, 9, kind, masks)
    want = O.twoview_cross_check(c.ocams[0], c.ocams[1], c.op, dl, dr)
    SM._upload(hip_ctx, c)
    got = {}
    for overlap in (1, 0):
        with SM._options(hip_ctx, tv_overlap=overlap):
            got[overlap] = hip_ctx.twoview_compute(0, 1, c.p)
        for k in range(2):
            SM._assert_depth(got[overlap][k], want[k], "%s tv_overlap=%d map %d" % (c.tag, overlap, k))
    for k in range(2):
        SM._assert_bits(got[1][k], got[0][k], "%s map %d, side by side against one after the other" % (c.tag, k))
    assert np.isfinite(want[0]).any()


@_params(C_PLANES)
def test_large_windows_by_products_against_the_oracle(hip_ctx, shape, radius, kind, masks, general):
    """winners, runners-up and both costs (twoview_winner_costs_kernel takes R at run time) against the oracle's diagnostics
    under the decision-gap rule; pair costs are refused at these radii"""
    c = SM._case(shape, radius, kind, masks)
    want = SM._oracle(shape, radius, kind, masks)
    for ref, oth, got in _planes_against_the_oracle(hip_ctx, c, want, WALK, ROWS_NCC):
        depth = hip_ctx.download_depth(ref)
        assert np.array_equal(np.isnan(depth), got["win_xy"][..., 0] < 0)


# Option "subpixel".  Measured on the CPU reference (tests/subpixel_ref.py): on all six inputs, in both directions, the
# reference's own numbers put NO pixel within the rule's distance of a class boundary, and every input has REFINED and
# NO_NEIGHBOUR pixels in the hundreds -- so only a pixel whose winner disagrees can be left out of the comparison.
SUBPIXEL_CASES = [("geodesic_r2", dict(radius=1)), ("geodesic_r2", dict(radius=3)), ("geodesic_r2", dict(radius=4)),
                  ("geodesic_r2", dict(radius=7)), ("adaptive_masks", dict(w=48, h=36, radius=9)),
                  ("geodesic_verged_dist_masks", dict(w=48, h=36, radius=6))]


@pytest.mark.parametrize("name,over", SUBPIXEL_CASES, ids=["%s-r%d" % (n, o["radius"]) for n, o in SUBPIXEL_CASES])
def test_subpixel_against_the_cpu_reference(hip_ctx, name, over):
    case = cases.get_twoview(name, **over)
    figures = SP.compare_with_the_cpu_reference(hip_ctx, "%s radius %d" % (name, over["radius"]), case)
    for left_out, counts in figures:
        assert counts[SR.REFINED] >= 100 and counts[SR.NO_NEIGHBOUR] >= 100, counts
    if over["radius"] <= 5:
        # (the replay fetches cm, c0, cp with srh_twoview_pair_costs, which stops at r = 5)
        p = SP._setup(hip_ctx, case)
        for ref, oth in DIRECTIONS:
            integer, got = SP._integer_and_refined(hip_ctx, p, ref, oth)
            assert not got["stats"]["used_dense_path"]
            counts = SP._replay(hip_ctx, case, p, ref, oth, got, integer)
            assert counts[SR.REFINED] > 0 and counts[SR.NO_NEIGHBOUR] > 0


# ------------------------------------------------------------------------------------------------ refusals
def _raises(code, fn, *a, **kw):
    with pytest.raises(capi.StereoHipError) as e:
        fn(*a, **kw)
    assert e.value.code == code, e.value


def _stage_calls(ctx, p):
    xy = np.array([[5, 5, 9, 5], [20, 12, 18, 12]], np.int32)
    return [("pair costs, SAD", lambda: ctx.twoview_pair_costs(0, 1, p, xy, capi.COST_SAD)),
            ("pair costs, NCC", lambda: ctx.twoview_pair_costs(0, 1, p, xy, capi.COST_NCC)),
            ("label costs", lambda: ctx.twoview_label_costs(0, 1, p)),
            ("mrf", lambda: ctx.twoview_mrf(0, 1, p)),
            ("sgm", lambda: ctx.twoview_sgm(0, 1, p)),
            ("compute_mrf", lambda: ctx.twoview_compute_mrf(0, 1, p)),
            ("compute_sgm", lambda: ctx.twoview_compute_sgm(0, 1, p))]


def test_what_is_refused_above_radius_5(hip_ctx):
    c = SM._case(MAIN, 6, 1)
    SM._upload(hip_ctx, c)
    before = [np.full((MAIN[1], MAIN[0]), -9.0 - k) for k in range(2)]
    for k in range(2):
        before[k][3, 4] = np.inf
        hip_ctx.upload_depth(k, before[k])
    calls = _stage_calls(hip_ctx, c.p) + [
        ("median", lambda: hip_ctx.filter_invalid(0, c.p, capi.FILTER_MEDIAN)),
        ("gaps + median", lambda: hip_ctx.filter_invalid(0, c.p, capi.FILTER_GAPS | capi.FILTER_MEDIAN))]
    for tag, call in calls:
        with pytest.raises(capi.StereoHipError) as e:
            call()
        assert e.value.code == capi.SRH_E_UNSUPPORTED, (tag, e.value)
        for k in range(2):
            SM._assert_bits(hip_ctx.download_depth(k), before[k], "depth map of slot %d after the refused %s" % (k, tag))
    # the same calls one radius lower are served
    p5 = capi.params_twoview(**dict(c.case["params"], window_radius=5))
    for tag, call in _stage_calls(hip_ctx, p5)[:3]:
        call()
    # the gap fill reads no window: it runs at r = 6, and matches tests/filter_ref.py
    w, h = 90, 70
    rgba, mask, depth = TF._synthetic(w, h, 0x5EED0F46)
    hip_ctx.upload_view(0, rgba, mask, TF._cam(w, h))
    got, info = TF._check(hip_ctx, 0, rgba, mask, depth, TF._params(6, 1), capi.FILTER_GAPS, tag="90x70 r6 gaps")
    assert info["gap_filled"] > 0
    _raises(capi.SRH_E_UNSUPPORTED, hip_ctx.filter_invalid, 0, TF._params(6, 1), capi.FILTER_MEDIAN)
    assert F.same_bits(hip_ctx.download_depth(0), got)


@pytest.mark.parametrize("radius", [0, 16])
def test_radii_outside_1_to_15_are_refused(hip_ctx, radius):
    c = SM._case(MAIN, 3, 1)
    SM._upload(hip_ctx, c)
    before = np.full((MAIN[1], MAIN[0]), -9.0)
    for k in range(2):
        hip_ctx.upload_depth(k, before)
    bad = capi.params_twoview(**dict(c.case["params"], window_radius=radius))
    calls = [("wta", lambda: hip_ctx.twoview_wta(0, 1, bad)), ("compute", lambda: hip_ctx.twoview_compute(0, 1, bad)),
             ("cross-check", lambda: hip_ctx.twoview_cross_check(0, 1, bad)),
             ("filter", lambda: hip_ctx.filter_invalid(0, bad, capi.FILTER_GAPS))] + _stage_calls(hip_ctx, bad)
    for tag, call in calls:
        with pytest.raises(capi.StereoHipError) as e:
            call()
        assert e.value.code == capi.SRH_E_INVALID, (tag, e.value)
    for k in range(2):
        SM._assert_bits(hip_ctx.download_depth(k), before, "depth map of slot %d" % k)
