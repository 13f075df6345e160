"""Every stereo path of the library on wide and tall views (tests/wide_shapes.py): 2049 .. M = capi.MAX_VIEW_DIM columns a
few rows high, the same turned on their side, and one wide view with a candidate range beyond the strip kernel's chunk.
What is under test are the 16-bit fields, the grid sizes and the index arithmetic at coordinates the rest of
the suite never reaches (it stops at 1920 x 1080).  One test is one shape.

Tolerances are the project's own: 1e-9 relative against the CPU oracle, bit equality between device paths, e0 of
capi.cert_bound for the fused cost rows.

Oracle times on the CPU, rows in bands on up to 16 threads (measured): one TwoView direction r = 5 geodesic 3.0 s at
32767x3x12, 1.0 s at 32767x2x8, 0.7 s at 8200x4x8, 0.5 s at 4097x6x8, below 0.3 s at every tall shape; 0.8 s at 8200x3x300
under wide_shapes.band_mask (12 s without it, for a single row: that shape meets the oracle under the mask only).
MultiViewStereo, one view: 0.5 .. 1.2 s at 2049x5x8 and 5x2049x8 (3.9 s on one thread); the estimate grows with the
square of the long side, so M x 5 and 5 x M compare the device's kernels with each other."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import cases
import fuse_ref
import mrf_cases
import oracle_ffi as O
import sad_ref as S
import test_gpu_cert_rows as CR
import test_gpu_filter as FT
import test_gpu_mrf as GM
import test_gpu_small_shapes as G
import test_gpu_twoview_mrf as TM
import test_gpu_wta_outputs as WO
import twoview_mrf_cases as TC
import twoview_mrf_ref as MR
import wide_shapes as WS
from stereoreconstruction_amd import capi

pytestmark = pytest.mark.gpu

M = WS.M
DIRECTIONS = G.DIRECTIONS
LONG = WS.LONG_RANGE_SHAPE
M_SHAPES = [s for s in WS.TWOVIEW_SHAPES if M in s[:2]]
_options, _assert_depth, _assert_bits = G._options, G._assert_depth, G._assert_bits
kinds = G.kinds


def _shapes(shapes):
    return pytest.mark.parametrize("shape", shapes, ids=WS.shape_id)


# (shape, masks) of the comparisons with the oracle: every shape plain and masked, LONG under its band mask only
ORACLE_CASES = [(s, m) for s in WS.TWOVIEW_SHAPES for m in (False, True) if m or s != LONG]
oracle_cases = pytest.mark.parametrize("shape,masks", ORACLE_CASES, ids=[WS.shape_id(s) + ("-masks" if m else "-plain") for s, m in ORACLE_CASES])


@functools.lru_cache(maxsize=None)
def _case(shape, radius, kind, masks=False, general=False):
    case = WS.wide_twoview(*shape, radius, kind, masks=masks, general=general)
    imgs, ocams, op = cases.oracle_inputs(case)
    cams, p = cases.hip_inputs(case)
    return types.SimpleNamespace(case=case, imgs=imgs, ocams=ocams, op=op, cams=cams, p=p, w=shape[0], h=shape[1],
                                 white=[v[1] == 1 for v in case["views"]], tag=case["name"])


@functools.lru_cache(maxsize=None)
def _oracle(shape, radius, kind, masks=False, general=False):
    """the CPU oracle's two passes, (depth, diag) each: computed once, shared, never written to"""
    c = _case(shape, radius, kind, masks, general)
    out = [WS.oracle_wta(O, c.imgs, c.ocams, c.op, r, o) for r, o in DIRECTIONS]
    for d, diag in out:
        d.setflags(write=False)
    return out


def _upload(ctx, c):
    cases.upload_case(ctx, c.case, c.cams)


def _edge(a, shape):
    """the last column of a wide view, the last row of a tall one"""
    return a[:, -1] if WS.is_wide(shape) else a[-1]


def _edge_name(shape):
    return "last column (x = %d)" % (shape[0] - 1) if WS.is_wide(shape) else "last row (y = %d)" % (shape[1] - 1)


def _assert_same_pass(d, planes, want_d, want_planes, shape, what):
    """depth map and winner planes of a pass, bit for bit: the far edge first, under its own message"""
    edge = _edge_name(shape)
    _assert_bits(_edge(d, shape), _edge(want_d, shape), "%s depth map, %s" % (what, edge))
    if planes is not None:
        WO._same_planes({k: _edge(v, shape) for k, v in planes.items()}, {k: _edge(v, shape) for k, v in want_planes.items()}, "%s, %s" % (what, edge))
        WO._same_planes(planes, want_planes, what)
    _assert_bits(d, want_d, what + " depth map")


# ---------------------------------------------------------------------------------------------- a. whole maps
@kinds
@oracle_cases
def test_whole_maps_against_the_oracle(hip_ctx, shape, masks, radius, kind):
    c = _case(shape, radius, kind, masks)
    want = _oracle(shape, radius, kind, masks)
    _upload(hip_ctx, c)
    for k, (ref, oth) in enumerate(DIRECTIONS):
        hip_ctx.twoview_wta(ref, oth, c.p)
        got, st = hip_ctx.download_depth(ref), hip_ctx.stats()
        depth, diag = want[k]
        print("%s %d>%d: finite %d, +INF %d, NaN %d, n_eval %d / %d" % (c.tag, ref, oth, np.isfinite(got).sum(), np.isposinf(got).sum(),
                                                                       np.isnan(got).sum(), st["n_eval"], diag["n_eval"]))
        _assert_depth(_edge(got, shape), _edge(depth, shape), "%s %d>%d, %s" % (c.tag, ref, oth, _edge_name(shape)))
        _assert_depth(got, depth, "%s %d>%d" % (c.tag, ref, oth))
        assert st["n_eval"] == diag["n_eval"], "%s %d>%d" % (c.tag, ref, oth)
        assert st["used_dense_path"] and np.isfinite(got).any()


# ---------------------------------------------------------------------------------------------- b. every rectified path
PATHS = G.PATHS
# (shape, path) the library declines, by a rule of the TwoView pass driver (TvPass::plan, twoview_wta_run; csrc/srh_api.hip) quoted here; the depth maps and planes
# of a declined pair are still the walk kernel's bits.  Only LONG declines anything, and that is what it is in the table for:
# its cstride is ((300 - 1) + 3 + 7) & ~7 = 304.
_CHUNK = "`cstride + SRH_WTILE <= strip_chunk_columns()`: 304 + 32 > 320, the per-tile kernel takes the pass"
DECLINES = {
    (LONG, "fused"): "`p->num_depth_levels <= SRH_FUSED_MAXC`: 300 labels, 256 cost-row columns in LDS",
    (LONG, "strip 4"): _CHUNK, (LONG, "strip 8"): _CHUNK, (LONG, "geodma 0 strip 4"): _CHUNK, (LONG, "geodma 0 strip 8"): _CHUNK,
}
SAD_DENSE_DECLINES = {LONG: "`sad && dense && cstride + SRH_WTILE > strip_chunk_columns()`: cost_sad has the strip form only, the lists take the pass"}


@kinds
@_shapes(WS.TWOVIEW_SHAPES)
def test_every_rectified_path_gives_the_walk_kernels_bits(hip_ctx, shape, radius, kind):
    c = _case(shape, radius, kind)
    _upload(hip_ctx, c)
    want = WO._yardstick(hip_ctx, c.p)
    for tag, opts, ran in PATHS:
        with _options(hip_ctx, wta_outputs=3, **opts):
            for k, (ref, oth) in enumerate(DIRECTIONS):
                d, got, st = WO._pass(hip_ctx, ref, oth, c.p)
                what = "%s %s %d>%d" % (c.tag, tag, ref, oth)
                if (shape, tag) in DECLINES:
                    assert not ran(st), "%s: listed as declined (%s), but the path ran: %s" % (what, DECLINES[(shape, tag)], st)
                else:
                    assert ran(st), "%s: the intended path did not run: %s" % (what, st)
                _assert_same_pass(d, got, want[k][0], want[k][1], shape, what)
    if shape == LONG:
        # by the host's choice: the defaults run the per-tile kernel here
        hip_ctx.twoview_wta(0, 1, c.p)
        st = hip_ctx.stats()
        assert st["used_dense_path"] and not st["used_strip_kernel"], st


def test_the_decline_table():
    """every entry names a shape and a path of the tables and a rule; no path is declined at every shape, none at a wide
    or tall shape of the ordinary candidate range"""
    for (shape, tag), rule in DECLINES.items():
        assert shape in WS.TWOVIEW_SHAPES and tag in [t for t, _, _ in PATHS] and rule
        assert shape == LONG
    for shape, rule in SAD_DENSE_DECLINES.items():
        assert shape == LONG and rule


# ---------------------------------------------------------------------------------------------- c. general geometry
def _profiled_pass(ctx, ref, oth, p):
    ctx.profile_reset()
    ctx.profile_enable(True)
    try:
        out = WO._pass(ctx, ref, oth, p)
    finally:
        ctx.synchronize()
        ctx.profile_enable(False)
    return out + (set(ctx.profile().keys()),)


@kinds
@_shapes(WS.GENERAL_SHAPES)
def test_general_geometry(hip_ctx, shape, radius, kind):
    """the row-run lists (the default of a verged pair), the lists in list order and the walk kernel against the oracle and
    against each other.  The rig keeps every curve within a few rows (wide_shapes.general_cameras), so the first pass of a
    pair after its upload has to STAND on the row-run kernels: they ran, and the plain list kernel did not take over."""
    c = _case(shape, radius, kind, False, True)
    want = _oracle(shape, radius, kind, False, True)
    _upload(hip_ctx, c)
    walk = WO._yardstick(hip_ctx, c.p)
    for k in range(2):
        _assert_depth(walk[k][0], want[k][0], "%s walk kernel, pass %d" % (c.tag, k))
        assert np.isfinite(walk[k][0]).mean() >= 0.5
    for tag, opts, ran in WO.GENERAL_PATHS:
        with _options(hip_ctx, wta_outputs=3, **opts):
            for k, (ref, oth) in enumerate(DIRECTIONS):
                d, got, st, launched = _profiled_pass(hip_ctx, ref, oth, c.p)
                what = "%s %s %d>%d" % (c.tag, tag, ref, oth)
                assert ran(st), "%s: the intended path did not run: %s" % (what, st)
                lists = sorted(n for n in launched if "rows" in n or "list" in n)
                if tag == "defaults":
                    assert "twoview_rows_list_kernel" in launched and "twoview_rows_scan_kernel" in launched and \
                        "twoview_list_kernel" not in launched, "%s: the row-run kernels did not take the pass: %s" % (what, lists)
                if tag == "list order":
                    assert "twoview_list_kernel" in launched and "twoview_rows_list_kernel" not in launched, "%s: %s" % (what, lists)
                assert st["n_eval"] == want[k][1]["n_eval"], what
                _assert_depth(_edge(d, shape), _edge(want[k][0], shape), "%s against the oracle, %s" % (what, _edge_name(shape)))
                _assert_depth(d, want[k][0], what + " against the oracle")
                _assert_same_pass(d, got, walk[k][0], walk[k][1], shape, what)


# ---------------------------------------------------------------------------------------------- d. SAD
def _sad_reference(c, ref, oth):
    from concurrent.futures import ThreadPoolExecutor
    bands = WS.row_bands(c.h)
    with ThreadPoolExecutor(max_workers=len(bands)) as ex:
        parts = list(ex.map(lambda b: S.twoview_wta_sad(c.imgs[ref], c.imgs[oth], c.ocams[ref], c.ocams[oth], c.op, b[0], b[1]), bands))
    out = parts[0]
    for (a, b), d in list(zip(bands, parts))[1:]:
        out[a:b] = d[a:b]
    return out


@pytest.mark.parametrize("radius,kind", [(2, 0)], ids=["r2_adaptive"])
@oracle_cases
def test_sad_maps_on_both_plans(hip_ctx, shape, masks, radius, kind):
    """(cost_sad reads no support weights beyond the window's size: one kind)"""
    c = _case(shape, radius, kind, masks)
    _upload(hip_ctx, c)
    want = [_sad_reference(c, r, o) for r, o in DIRECTIONS]
    got = {}
    for sad_dense in (0, 1):
        with _options(hip_ctx, cost=capi.COST_SAD, sad_dense=sad_dense):
            for k, (ref, oth) in enumerate(DIRECTIONS):
                hip_ctx.twoview_wta(ref, oth, c.p)
                st = hip_ctx.stats()
                what = "%s sad_dense=%d %d>%d" % (c.tag, sad_dense, ref, oth)
                dense = bool(sad_dense) and shape not in SAD_DENSE_DECLINES
                assert bool(st["used_dense_path"]) == dense, "%s: %s" % (what, st)
                got[sad_dense, k] = hip_ctx.download_depth(ref)
                _assert_bits(_edge(got[sad_dense, k], shape), _edge(want[k], shape), "%s, %s" % (what, _edge_name(shape)))
                _assert_bits(got[sad_dense, k], want[k], what)
    for k in range(2):
        _assert_bits(got[1, k], got[0, k], "%s dense against lists, pass %d" % (c.tag, k))
        assert np.isfinite(want[k]).any()


# ---------------------------------------------------------------------------------------------- e. both passes + cross-check
COMPUTE_CASES = [(s, m) for s, m in ORACLE_CASES if s in M_SHAPES + [(8200, 4, 8)] and not m]


@kinds
@pytest.mark.parametrize("shape,masks", COMPUTE_CASES, ids=[WS.shape_id(s) for s, m in COMPUTE_CASES])
def test_compute_against_the_oracles_passes_and_cross_check(hip_ctx, shape, masks, radius, kind):
    c = _case(shape, radius, kind, masks)
    (dl, _), (dr, _) = _oracle(shape, radius, kind, masks)
    want = O.twoview_cross_check(c.ocams[0], c.ocams[1], c.op, dl, dr)
    _upload(hip_ctx, c)
    for overlap in (1, 0):
        with _options(hip_ctx, tv_overlap=overlap):
            got = hip_ctx.twoview_compute(0, 1, c.p)
        for k in range(2):
            _assert_depth(_edge(got[k], shape), _edge(want[k], shape), "%s tv_overlap=%d map %d, %s" % (c.tag, overlap, k, _edge_name(shape)))
            _assert_depth(got[k], want[k], "%s tv_overlap=%d map %d" % (c.tag, overlap, k))
    assert np.isfinite(want[0]).any() and np.isfinite(want[1]).any()


# ---------------------------------------------------------------------------------------------- f. cost rows
ROWS_SHAPES = WS.WIDE_SHAPES + [LONG]


def _strips(shape):
    return (0,) if (shape, "strip 4") in DECLINES else (0, 4, 8)


@pytest.mark.parametrize("masks", [False, True], ids=["plain", "masks"])
@kinds
@_shapes(ROWS_SHAPES)
def test_fused_cost_rows_within_the_bound(hip_ctx, shape, radius, kind, masks):
    c = _case(shape, radius, kind, masks)
    _upload(hip_ctx, c)
    for strip in _strips(shape):
        tag = "%s strip=%d" % (c.tag, strip)
        worst, n_cert, n_clamp, n_unc = CR._rows_check(hip_ctx, c.p, 0, c.h, strip, tag)
        print("cost rows %s: max |fused - exact| = %.3g e0 over %d certified entries (%d clamps, %d uncertified)" % (tag, worst, n_cert, n_clamp, n_unc))
        assert n_cert > 0, tag


@pytest.mark.parametrize("masks", [False, True], ids=["plain", "masks"])
@kinds
@_shapes(ROWS_SHAPES)
def test_exact_cost_rows_against_the_oracle(hip_ctx, shape, radius, kind, masks):
    """every live entry of the rows in the reference's arithmetic is the oracle's cost of (pixel, lo + k), in all three
    kernel forms -- entry by entry at the pixels of wide_shapes.sample_columns (a row of 32767 pixels has 400 000 entries:
    the oracle is asked for those at either end of the rows and around every power of two, where an address could go wrong),
    and on the whole rows the three forms agree bit for bit"""
    c = _case(shape, radius, kind, masks)
    _upload(hip_ctx, c)
    cols = np.array(WS.sample_columns(c.w, 35 if shape[2] <= 16 else 4))
    L = O.lib()
    known = {}

    def oracle_cost(y, x, cx, wts):
        if (y, x, cx) not in known:
            known[y, x, cx] = L.sro_twoview_cost_ncc(C.byref(c.imgs[0].c), C.byref(c.imgs[1].c), O.dptr(wts[y, x]), C.byref(c.op), x, y, cx, y)
        return known[y, x, cx]
    wts = {}
    first = None
    for strip in _strips(shape):
        tag = "%s strip=%d" % (c.tag, strip)
        hip_ctx.set_option("strip", strip)
        try:
            exact, rng, us = hip_ctx.twoview_cost_rows(0, 1, c.p, 0, c.h, 0)
        finally:
            hip_ctx.set_option("strip", 1)
        assert us == (strip != 0), tag
        nonempty = rng[..., 1] >= rng[..., 0]
        assert (rng[..., 0][nonempty] >= 0).all() and (rng[..., 1][nonempty] < c.w).all(), tag
        assert rng[..., 1].max() >= c.w - 2, tag                           # left to right the last candidate is column w - 2
        assert (rng[..., 1] - rng[..., 0] + 1).max() <= exact.shape[2], tag
        live = CR._valid(rng, exact.shape[2]) & (exact.view(np.uint64) != CR.UNWRITTEN)
        if first is None:
            first = (exact, live)
        else:
            assert np.array_equal(live, first[1]) and np.array_equal(exact.view(np.uint64)[live], first[0].view(np.uint64)[live]), tag + ": not the bits of strip=0"
        sel = np.zeros(live.shape, bool)
        sel[:, cols] = live[:, cols]
        ys, xs, ks = np.nonzero(sel)
        for y, x in set(zip(ys.tolist(), xs.tolist())):
            if (y, x) not in wts:
                wts[y, x] = np.ascontiguousarray(O.weights(c.imgs[0], x, y, c.op), dtype=np.float64)
        want = np.array([oracle_cost(int(y), int(x), int(rng[y, x, 0] + k), wts) for y, x, k in zip(ys, xs, ks)])
        ok = WO._close(exact[ys, xs, ks], want)
        print("%s: cstride %d, %d live entries, %d of them against the oracle, %d off" % (tag, exact.shape[2], live.sum(), len(ys), (~ok).sum()))
        assert ok.all(), "%s: %d of %d entries, first (y, x, k) %s: got %r want %r" % (
            tag, (~ok).sum(), len(ys), [int(a[~ok][0]) for a in (ys, xs, ks)], exact[ys, xs, ks][~ok][0], want[~ok][0])
        assert len(ys) > 0 and xs.max() >= c.w - 35, tag


# ---------------------------------------------------------------------------------------------- g. hole filling, label costs, TRW-S
@pytest.mark.parametrize("w,h", [(M, 3), (3, M)], ids=["%dx3" % M, "3x%d" % M])
def test_hole_filling(hip_ctx, w, h):
    rgba, _, depth = FT._synthetic(w, h, 0x5EED0F40 + w)
    # (_synthetic's ragged mask starts w / 16 + up to 36 columns in: nothing of a view 3 columns wide; here 2 % masked out)
    mask = (np.random.default_rng(w).random((h, w)) >= 0.02).astype(np.uint8)
    # holes along the far edge: its last 6 columns / rows, +INF and NaN by turns, a pixel in 7 left standing
    far = depth[:, -6:] if w > h else depth[-6:].T
    along = np.arange(far.shape[0])
    for k in range(6):
        far[:, k] = np.where((along + k) % 7 == 0, far[:, k], np.where((along + k) % 2 == 0, np.inf, np.nan))
    hip_ctx.upload_view(0, rgba, mask, FT._cam(w, h))
    for radius, kind in WS.TWOVIEW_KINDS:
        got, info = FT._check(hip_ctx, 0, rgba, mask, depth, FT._params(radius, kind), 3, tag="%dx%d r%d k%d" % (w, h, radius, kind))
        edge = (slice(None), slice(-6, None)) if w > h else (slice(-6, None), slice(None))
        white = mask[edge] == 1
        filled = white & ~np.isfinite(depth[edge]) & np.isfinite(got[edge])
        print("%dx%d r%d k%d: %s; filled along the far edge %d of %d holes" % (w, h, radius, kind, info, filled.sum(), (white & ~np.isfinite(depth[edge])).sum()))
        assert info["holes"] > 0.2 * w * h and info["median_filled"] > 0 and filled.sum() > 0


@kinds
def test_label_costs(hip_ctx, radius, kind):
    shape = (8200, 3, 4)
    c = _case(shape, radius, kind)
    _upload(hip_ctx, c)
    fill = MR.fill_value(c.p.window_radius, c.p.bad_ret)
    for ref, oth in DIRECTIONS:
        want_pix = TM._cpu_label_pixels(c.case, c.ocams, c.op, ref, oth)
        has = want_pix[..., 0] != TM.NONE
        assert has[:, -1].any() or has[:, 0].any()
        yy, xx, dd = np.nonzero(has)
        assert xx.max() >= c.w - 2 and want_pix[..., 0].max() >= c.w - 2
        xy = np.stack([xx, yy, want_pix[yy, xx, dd, 0], want_pix[yy, xx, dd, 1]], 1).astype(np.int32)
        for cost_kind, kname in ((capi.COST_NCC, "ncc"), (capi.COST_SAD, "sad")):
            tag = "%s %s %d>%d" % (c.tag, kname, ref, oth)
            with _options(hip_ctx, cost=cost_kind):
                cost, pix = hip_ctx.twoview_label_costs(ref, oth, c.p)
                assert np.array_equal(pix, want_pix), "%s: %d label pixels differ" % (tag, (pix != want_pix).any(axis=-1).sum())
                assert (cost[~has] == fill).all(), tag
                pc = hip_ctx.twoview_pair_costs(ref, oth, c.p, xy, cost_kind)
                _assert_bits(cost[yy, xx, dd], pc, tag + " vs pair costs")
                sub = np.concatenate([np.arange(0, len(xy), max(1, len(xy) // 200)), np.nonzero(xx >= c.w - 3)[0]])
                if cost_kind == capi.COST_SAD:
                    TM._assert_costs(pc[sub], S.pair_costs_sad(c.imgs[ref], c.imgs[oth], c.op, xy[sub]), tag + " oracle")
                else:
                    TM._assert_costs(pc[sub], S.pair_costs_ncc(c.imgs[ref], c.imgs[oth], c.op, xy[sub]), tag + " oracle", rtol=1e-9)
                for y in range(c.h):
                    band, bpix = hip_ctx.twoview_label_costs(ref, oth, c.p, y, y + 1)
                    _assert_bits(band, cost[y:y + 1], "%s row %d" % (tag, y))
                    assert np.array_equal(bpix, pix[y:y + 1]), "%s row %d" % (tag, y)


TRWS_GRIDS = [(8200, 3), (3, 8200)]


@pytest.mark.parametrize("w,h", TRWS_GRIDS, ids=["%dx%d" % g for g in TRWS_GRIDS])
def test_twoview_trws_fixed_sweeps(hip_ctx, w, h):
    """L = 4; 3 x 8200 is 513 bands of 16 rows handing over to each other, 8200 x 3 one band 8200 steps long"""
    for integer in (False, True):
        costs, mask = TC.volume(w, h, 4, seed=w * 131 + h + 4, integer=integer)
        info, _ = TM._check_optimizer(hip_ctx, costs, mask, dict(min_energy_drop=-1.0, max_iters=2), "3 sweeps %dx%dx4%s" % (w, h, " int" if integer else ""))
        assert info["iterations"] == 3


@pytest.mark.parametrize("w,h", TRWS_GRIDS, ids=["%dx%d" % g for g in TRWS_GRIDS])
def test_mvs_trws_fixed_sweeps(hip_ctx, w, h):
    peaks, mask = mrf_cases.peaks_case(w, h, K=4, seed=w * 131 + h, fill=0.6)
    info, _ = GM._check_against_oracle(hip_ctx, peaks, mask, dict(min_energy_drop=-1.0, max_iters=2), "3 sweeps %dx%d" % (w, h))
    assert info["iterations"] == 3


# ---------------------------------------------------------------------------------------------- h. MultiViewStereo
@functools.lru_cache(maxsize=None)
def _mvs(shape, kind, oracle):
    case = WS.wide_mvs(*shape, kind)
    imgs, ocams, op = cases.oracle_inputs(case)
    neigh = [[int(n) for n in v] for v in O.mvs_neighbours(ocams, op)]
    want = [WS.oracle_mvs(O, imgs, ocams, v, neigh[v], op) for v in range(3)] if oracle else None
    cams, p = cases.hip_inputs(case)
    return types.SimpleNamespace(case=case, imgs=imgs, ocams=ocams, op=op, cams=cams, p=p, neigh=neigh, want=want, tag=case["name"],
                                 masks=[v[1] for v in case["views"]])


def _mvs_modes(ctx, c, shape):
    """the three views under the defaults (staged cost kernel), with mvs_staged = 0 (gathering kernel) and on the inline
    one-thread-per-pixel kernel: the same bits and counts, and each stat shows that its kernel took waves"""
    out = {}
    for tag, opts in (("default", {}), ("gathering", dict(mvs_staged=0)), ("inline", dict(force_generic=1))):
        with _options(ctx, **opts):
            maps, evals, staged, listed = [], [], 0, 0
            for v in range(3):
                ctx.mvs_initial_estimate(v, c.neigh[v], c.p)
                st = ctx.stats()
                maps.append(ctx.download_depth(v))
                evals.append(st["n_eval"])
                staged += st["mvs_waves_staged"]
                listed += st["mvs_waves_listed"]
        print("%s %s: n_eval %s, waves staged %d, listed %d" % (c.tag, tag, evals, staged, listed))
        # (a window box fits a view 5 columns wide only where all 64 candidates of a wave lie in its middle column: the
        # waves of a tall view go to the gathering kernel, those of a wide one are staged; with mvs_staged = 0 the walk
        # kernel makes no window descriptors and counts neither kind, tests/test_gpu_small_shapes.py)
        if tag == "default":
            assert (staged > 0) if WS.is_wide(shape) else (listed > 0), (c.tag, tag, staged, listed)
        if tag == "gathering":
            assert staged == 0, (c.tag, tag)
        out[tag] = (maps, evals)
    for v in range(3):
        for tag in ("gathering", "inline"):
            _assert_bits(_edge(out[tag][0][v], shape), _edge(out["default"][0][v], shape), "%s view %d %s against the defaults, %s" % (c.tag, v, tag, _edge_name(shape)))
            _assert_bits(out[tag][0][v], out["default"][0][v], "%s view %d %s against the defaults" % (c.tag, v, tag))
            assert out[tag][1][v] == out["default"][1][v], (c.tag, v, tag)
        assert np.isposinf(out["default"][0][v][c.masks[v] != 1]).all() and np.isfinite(out["default"][0][v]).any()
    return out["default"]


@pytest.mark.parametrize("kind", [1, 0], ids=["geodesic", "adaptive"])
@_shapes(WS.MVS_ORACLE_SHAPES)
def test_mvs_against_the_oracle(hip_ctx, shape, kind):
    c = _mvs(shape, kind, True)
    assert capi.mvs_neighbours(c.cams, c.p) == c.neigh
    _upload(hip_ctx, c)
    maps, evals = _mvs_modes(hip_ctx, c, shape)
    for v in range(3):
        _assert_depth(maps[v], c.want[v][0], "%s view %d" % (c.tag, v))
        assert evals[v] == c.want[v][1], (c.tag, v)
    # the cross-check in view order, each view reading the already filtered earlier views
    ref = [np.array(d) for d, _ in c.want]
    for v in range(3):
        O.mvs_cross_check(c.imgs, c.ocams, v, c.op, ref)
    for v in range(3):
        hip_ctx.upload_depth(v, np.array(c.want[v][0]))
    for v in range(3):
        hip_ctx.mvs_cross_check([0, 1, 2], v, c.p)
    for v in range(3):
        _assert_depth(hip_ctx.download_depth(v), ref[v], "%s view %d cross-check" % (c.tag, v))


@_shapes(WS.MVS_DEVICE_SHAPES)
def test_mvs_device_kernels_agree(hip_ctx, shape):
    c = _mvs(shape, 1, False)
    _upload(hip_ctx, c)
    maps, evals = _mvs_modes(hip_ctx, c, shape)
    assert min(evals) > 0
    # candidates up to the far end of the long side: the lists hold coordinates up to M - 1
    long_axis = 1 if WS.is_wide(shape) else 0
    assert max(np.nonzero(np.isfinite(m))[long_axis].max() for m in maps) > 0.55 * M


def test_mvs_fuse(hip_ctx):
    """at the largest MultiViewStereo shape the oracle checks: 2049 x 5"""
    w, h, D = WS.MVS_ORACLE_SHAPES[0]
    over = dict(nviews=3, w=w, h=h, D=D)
    I = fuse_ref.case_inputs("mvs_geodesic", **over)
    want = fuse_ref.case_result("mvs_geodesic", **over)
    cams, p = cases.hip_inputs(I["case"])
    for v in range(3):
        hip_ctx.upload_view(v, I["case"]["views"][v][0], I["case"]["views"][v][1], cams[v])
        hip_ctx.upload_depth(v, I["depths"][v])
    got = hip_ctx.mvs_fuse([0, 1, 2], p, capi.fuse_params(dist_threshold=I["thr"]))
    fuse_ref.assert_equal(got, want, "2049x5", [m.size for m in I["masks"]])
    assert got["n_points"] > 1000 and got["n_claimed"] > 0


# ---------------------------------------------------------------------------------------------- i. the limit
def _blank(w, h, seed=0):
    rgba = np.zeros((h, w, 4), np.uint8)
    rgba[..., :3] = ((np.arange(w)[None, :, None] * 7 + np.arange(h)[:, None, None] * 13 + np.arange(3) + seed) % 251).astype(np.uint8)
    rgba[..., 3] = 255
    return rgba


def _refused(call):
    with pytest.raises(capi.StereoHipError) as e:
        call()
    assert e.value.code == capi.SRH_E_UNSUPPORTED, e.value
    return e.value


def test_upload_refuses_beyond_the_limit(hip_ctx):
    slot = 5
    rgba = _blank(37, 11, seed=3)
    mask = (np.arange(37)[None, :] + np.arange(11)[:, None]) % 5 != 0
    hip_ctx.upload_view(slot, rgba, mask.astype(np.uint8), FT._cam(37, 11))
    before = hip_ctx.download_view_image(slot)
    cam = FT._cam(64, 64)
    for w, h in ((M + 1, 1), (1, M + 1), (M + 1, M + 1), (40000, 4), (3, 40000)):
        big = np.zeros((1, 1, 4), np.uint8)
        # (the refusal comes before a byte is read: a 1 x 1 buffer stands for the M + 1 squared image)
        rc = capi.lib().srh_view_upload(hip_ctx._h, slot, w, h, big.ctypes.data_as(capi.c_uint8_p), None, C.byref(cam))
        assert rc == capi.SRH_E_UNSUPPORTED, (w, h, rc)
    _refused(lambda: hip_ctx.upload_view(slot, _blank(M + 1, 1), None, cam))
    _refused(lambda: hip_ctx.upload_view(slot, _blank(1, M + 1), None, cam))
    # scaled: the identity of a source beyond the limit, and strict downscales whose target is beyond it, wide and tall
    _refused(lambda: hip_ctx.upload_view_scaled(slot, _blank(M + 1, 2), False, 1.0, cam))
    _refused(lambda: hip_ctx.upload_view_scaled(slot, _blank(70000, 2), False, 0.5, cam))
    _refused(lambda: hip_ctx.upload_view_scaled(slot, _blank(2, 70000), False, 0.5, cam))
    assert hip_ctx.view_size(slot) == (37, 11)
    after = hip_ctx.download_view_image(slot)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # ... and a scaled upload whose target is just inside goes through
    hip_ctx.upload_view_scaled(slot, _blank(2 * M, 2), False, 0.5, cam)
    assert hip_ctx.view_size(slot) == (M, 1)


@pytest.mark.parametrize("shape", [(M, 1, 8), (1, M, 2)], ids=WS.shape_id)
def test_views_at_the_limit_upload_and_equal_the_oracle(hip_ctx, shape):
    for radius, kind in WS.TWOVIEW_KINDS:
        c = _case(shape, radius, kind)
        want = _oracle(shape, radius, kind)
        _upload(hip_ctx, c)
        assert hip_ctx.view_size(0) == hip_ctx.view_size(1) == shape[:2]
        for k, (ref, oth) in enumerate(DIRECTIONS):
            hip_ctx.twoview_wta(ref, oth, c.p)
            _assert_depth(hip_ctx.download_depth(ref), want[k][0], "%s %d>%d" % (c.tag, ref, oth))
            assert hip_ctx.stats()["n_eval"] == want[k][1]["n_eval"]
        assert np.isfinite(want[0][0]).any()
