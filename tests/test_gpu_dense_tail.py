"""The fixed-cost kernels at the ends of the dense TwoView pass ("dense tail"):

  * the left-out columns come from a LIST that pixel_range_kernel makes (band.filllist) and the fill kernels loop over;
  * the certified redo of the flagged pixels is ONE kernel (twoview_redo_kernel: the cost columns beside the walk), the pair
    refill + one-lane scan where it is not eligible;
  * label table, scan template and range kernel run on the context's side stream beside the windows kernel (option
    side_weights), one side stream for both passes of srh_twoview_compute.

None of them changes a bit: everything here is compared with the CPU oracle, with the reference's arithmetic on the device
or with a fresh context."""
import numpy as np
import pytest

from stereoreconstruction_amd import capi, synthetic
import test_gpu_arith_modes as am
import test_gpu_cert_rows as cr

pytestmark = pytest.mark.gpu

REDO_GRID = 512          # RD_GRID of srh_dense.hip: the redo kernel's workgroups


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class _Options:
    """set options for a block, put the library's defaults back afterwards"""
    DEFAULTS = dict(arith=capi.ARITH_DEFAULT, strip=1, band_budget_mb=32768, wta_outputs=0, tv_overlap=1, side_weights=1,
                    cost=capi.COST_NCC, sad_dense=0)

    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.ctx.set_option(k, self.DEFAULTS[k])


# ------------------------------------------------------------------------------------------------------ fill list
FILL_W, FILL_H = 160, 24
# A pixel's column range is as wide as the label count away from the left image border and grows from nothing to that
# at the border; the cost kernel leaves a pixel's last one or two columns out where its range is one or two columns more
# than a whole multiple of 8 * lanes columns (dense_cover_hi: lanes = 8, or 4 in the 4-wave strip form).
#   24: no range reaches 33 columns -- nothing is left out in any form, the list stays empty;
#   64: the ranges away from the border are whole multiples (+ the walk's margin), those at the border pass 33 / 34;
#   72: 65 / 66 columns only at the border, where the ranges grow through them.
FILL_LABELS = [24, 64, 72]
_fill_cache = {}


def _fill_pair(D):
    """the pair (masks with holes), its parameters and the oracle's maps, made once per label count"""
    if D not in _fill_cache:
        import cases
        import oracle_ffi as O
        case = cases.get_twoview("geodesic_masks", w=FILL_W, h=FILL_H, D=D)
        imgs, ocams, op = cases.oracle_inputs(case)
        dl, diag = O.twoview_wta(imgs[0], imgs[1], ocams[0], ocams[1], op, want_diag=True)
        dr = O.twoview_wta(imgs[1], imgs[0], ocams[1], ocams[0], op)
        cl, cr_ = O.twoview_cross_check(ocams[0], ocams[1], op, dl, dr)
        for a in (dl, dr, cl, cr_, diag["win_xy"], diag["min_cost"]):
            a.setflags(write=False)
        _fill_cache[D] = dict(case=case, wta=(dl, dr), checked=(cl, cr_), diag=diag)
    return _fill_cache[D]


def _upload(ctx, case):
    import cases
    cams, p = cases.hip_inputs(case)
    cases.upload_case(ctx, case, cams)
    return p


def _left_out(rng, lanes, pad):
    """pixels whose last columns dense_cover_hi(lo, hi, 8, lanes, pad) leaves out, from the ranges the device returned"""
    lo, hi = rng[..., 0].astype(np.int64), rng[..., 1].astype(np.int64)
    lo_e = np.where(pad, lo & ~1, lo)
    nblocks = (hi - lo_e + 8) // 8
    last = (hi - lo_e + 1) - (nblocks - 1) * 8
    return int(((hi >= lo) & (nblocks > lanes) & (nblocks % lanes == 1) & (last <= 2)).sum())


def _assert_depth(got, want, tag):
    import cases
    ok, msg, _ = cases.compare_depth(got, want, 1e-9)
    assert ok, "%s: %s" % (tag, msg)


@pytest.mark.parametrize("strip", [8, 4, 0])
@pytest.mark.parametrize("D", FILL_LABELS)
def test_fill_list_cost_rows_are_complete(hip_ctx, D, strip):
    """srh_twoview_cost_rows, forms 0 and 5, the whole image and the row range [5, 17): every column of every masked-in
    pixel's range is written (the call fills the rows with NaNs of payload -1 first), form 5 is within the bound of form 0,
    and form 0 at the oracle's winner is the oracle's minimum cost."""
    pair = _fill_pair(D)
    p = _upload(hip_ctx, pair["case"])
    e0 = capi.cert_bound(p)["e0"]
    with _Options(hip_ctx, strip=strip):
        for y0, y1 in ((0, FILL_H), (5, 17)):
            exact, rng, us = hip_ctx.twoview_cost_rows(0, 1, p, y0, y1, 0)
            assert us == (strip != 0)
            valid = cr._valid(rng, exact.shape[2])
            assert valid.any()
            assert not (_bits(exact)[valid] == cr.UNWRITTEN).any(), "form 0, rows %d..%d: an entry of a pixel's range was never written" % (y0, y1)
            fused, rng2, _ = hip_ctx.twoview_cost_rows(0, 1, p, y0, y1, 5)
            assert np.array_equal(rng, rng2)
            assert not (_bits(fused)[valid] == cr.UNWRITTEN).any(), "form 5, rows %d..%d: an entry of a pixel's range was never written" % (y0, y1)
            ratio, _, _, n_unc, _ = cr._compare(exact, fused, valid, p, e0, "D %d strip %d rows %d..%d" % (D, strip, y0, y1))
            assert ratio <= 1.0 and (n_unc == 0 or strip == 0)
            # the oracle's winner and its cost, in the device's cost row
            win, mc = pair["diag"]["win_xy"][y0:y1], pair["diag"]["min_cost"][y0:y1]
            has = (win[..., 0] >= 0) & (rng[..., 1] >= rng[..., 0])
            k = (win[..., 0] - rng[..., 0])[has]
            assert (win[..., 1][has] == np.nonzero(has)[0] + y0).all() and (k >= 0).all() and (k < exact.shape[2]).all()
            got = exact[has][np.arange(k.size), k]
            # (the parity rule of cases.compare_depth: 1e-9 * max(1, |value|); costs are O(1) and 0 for a perfect match)
            assert np.allclose(got, mc[has], rtol=1e-9, atol=1e-9),"form 0 against the oracle's minimum costs: max difference %.3g" % np.abs(got - mc[has]).max()
            n8, n4 = _left_out(rng, 8, True), _left_out(rng, 4, False)
            print("fill list D %d strip %d rows %d..%d: pixels with left-out columns -- 8 lanes, even blocks: %d; 4 lanes: %d; 8 lanes: %d"
                  % (D, strip, y0, y1, n8, n4, _left_out(rng, 8, False)))
            if D == 24:
                assert n8 == 0 and n4 == 0
            if D == 72:
                assert n8 > 0, "ranges that grow through 65 / 66 columns at the border must leave columns out"


@pytest.mark.parametrize("D", FILL_LABELS)
def test_fill_list_depth_maps_equal_the_oracle(hip_ctx, D):
    """Both directions and the cross-check, strip 8 / 4 / 0, in one band, in bands of a few rows and as a row range; in the
    reference's arithmetic the device evaluates the same number of candidates in every form."""
    pair = _fill_pair(D)
    p = _upload(hip_ctx, pair["case"])
    n_dev = {}
    for strip in (8, 4, 0):
        for budget in (32768, 1):
            with _Options(hip_ctx, strip=strip, band_budget_mb=budget):
                gl, gr = hip_ctx.twoview_compute(0, 1, p)
                tag = "D %d strip %d budget %d MB" % (D, strip, budget)
                _assert_depth(gl, pair["checked"][0], tag + " left")
                _assert_depth(gr, pair["checked"][1], tag + " right")
                hip_ctx.twoview_wta(0, 1, p)
                _assert_depth(hip_ctx.download_depth(0), pair["wta"][0], tag + " left, before the cross-check")
        with _Options(hip_ctx, strip=strip):
            # rows [5, 17) only: the rows outside keep what the pass above left there
            before = hip_ctx.download_depth(0)
            hip_ctx.twoview_wta(0, 1, p, 5, 17)
            after = hip_ctx.download_depth(0)
            assert np.array_equal(_bits(before), _bits(after)), "D %d strip %d: the row range changed the map" % (D, strip)
        with _Options(hip_ctx, strip=strip, arith=capi.ARITH_EXACT):
            hip_ctx.twoview_wta(0, 1, p)
            n_dev[strip] = hip_ctx.stats()["n_eval_device"]
            _assert_depth(hip_ctx.download_depth(0), pair["wta"][0], "D %d strip %d exact" % (D, strip))
    print("fill list D %d: n_eval_device in the reference's arithmetic, strip 8 / 4 / 0: %s" % (D, n_dev))
    assert n_dev[8] == n_dev[4] == n_dev[0] > 0


# ------------------------------------------------------------------------------------------------------ redo
def _redo_pair(ctx, kind, W, H, D):
    if kind == "textured":
        L, R, ml, mr, _ = synthetic.rectified_pair(W, H, D, 0x5EED0A07)
    else:
        L, R, ml, mr = am._adversarial_pair(kind, W, H, D)
    (Kl, Rl, tl), (Kr, Rr, tr) = synthetic.rectified_cameras(W, H)
    zmin, zmax = synthetic.rectified_depth_range(W, D)
    ctx.upload_view(0, L, ml, capi.camera_from_krt(Kl, Rl, tl))
    ctx.upload_view(1, R, mr, capi.camera_from_krt(Kr, Rr, tr))
    return capi.params_twoview(min_depth=zmin, max_depth=zmax, num_depth_levels=D, weight_kind=capi.WEIGHT_GEODESIC)


def _passes(ctx, p, arith, y0=0, y1=0, wta=False):
    """-> per direction (depth bits, stats, WTA planes or None), then the cross-checked maps' bits"""
    out = []
    with _Options(ctx, arith=arith):
        for a, b in ((0, 1), (1, 0)):
            ctx.twoview_wta(a, b, p, y0, y1)
            out.append((_bits(ctx.download_depth(a)).copy(), ctx.stats(), ctx.wta_outputs(a) if wta else None))
        ctx.twoview_cross_check(0, 1, p)
        out.append((_bits(ctx.download_depth(0)).copy(), _bits(ctx.download_depth(1)).copy()))
    return out


def _assert_same(exact, cert, tag, wta=False):
    for d in range(2):
        assert np.array_equal(exact[d][0], cert[d][0]), "%s direction %d: %d depths differ" % (tag, d, (exact[d][0] != cert[d][0]).sum())
        assert cert[d][1]["n_certified"] == cert[d][1]["n_pixels"] > 0, (tag, cert[d][1])
        if wta:
            for k in ("win_xy", "runner_xy"):
                assert np.array_equal(exact[d][2][k], cert[d][2][k]), "%s direction %d: %s differs" % (tag, d, k)
    assert np.array_equal(exact[2][0], cert[2][0]) and np.array_equal(exact[2][1], cert[2][1]), tag + ": after the cross-check"


# (the periodic pair flags four pixels in five -- 14 620 and 14 705 of 18 432 at 192 x 96, printed below: already there
# every workgroup of the redo kernel takes dozens of pixels; 64 x 12: a short list, a pixel or two per workgroup)
@pytest.mark.parametrize("kind,W,H,D", [("textured", 192, 96, 40), ("periodic", 192, 96, 40), ("periodic", 64, 12, 40)],
                         ids=["textured", "periodic-looping", "periodic-small"])
def test_redo_certified_equals_exact(hip_ctx, kind, W, H, D):
    p = _redo_pair(hip_ctx, kind, W, H, D)
    with _Options(hip_ctx, strip=8):
        exact = _passes(hip_ctx, p, capi.ARITH_EXACT)
        cert = _passes(hip_ctx, p, capi.ARITH_CERTIFIED)
        _assert_same(exact, cert, "%s %dx%d" % (kind, W, H))
        flagged = [cert[d][1]["n_flagged"] for d in range(2)]
        print("redo %s %dx%dx%d: flagged per direction %s of %d pixels" % (kind, W, H, D, flagged, W * H))
        if kind == "textured":
            assert flagged == [0, 0]
        else:
            assert min(flagged) > 0
        if kind == "periodic" and (W, H) == (192, 96):
            assert min(flagged) > REDO_GRID, "the redo kernel's workgroups must take more than one pixel each here"


def test_redo_variants(hip_ctx):
    """the periodic pair with the WTA by-products kept, in bands of a row or two, and over a row range"""
    W, H, D = 192, 96, 40
    p = _redo_pair(hip_ctx, "periodic", W, H, D)
    with _Options(hip_ctx, strip=8, wta_outputs=1):
        _assert_same(_passes(hip_ctx, p, capi.ARITH_EXACT, wta=True), _passes(hip_ctx, p, capi.ARITH_CERTIFIED, wta=True), "wta_outputs", wta=True)
    with _Options(hip_ctx, strip=8):
        whole = _passes(hip_ctx, p, capi.ARITH_EXACT)
        with _Options(hip_ctx, band_budget_mb=1):
            banded = _passes(hip_ctx, p, capi.ARITH_CERTIFIED)
        _assert_same(whole, banded, "bands")
        assert min(banded[d][1]["n_flagged"] for d in range(2)) > 0
        # a row range (the rows outside keep what the cross-check above left there: only the range is compared)
        ranged = _passes(hip_ctx, p, capi.ARITH_CERTIFIED, 21, 58)
        for d in range(2):
            assert np.array_equal(whole[d][0][21:58], ranged[d][0][21:58]), "row range, direction %d" % d
            assert 0 < ranged[d][1]["n_pixels"] <= (58 - 21) * W
            assert ranged[d][1]["n_flagged"] > 0


def test_redo_fallback_pair_beyond_the_label_limit(hip_ctx):
    """1030 labels (more than RSW_MAXD): refill + one-lane scan"""
    W, H, D = 64, 12, 1030
    p = _redo_pair(hip_ctx, "periodic", W, H, D)
    with _Options(hip_ctx, strip=8):
        exact = _passes(hip_ctx, p, capi.ARITH_EXACT)
        cert = _passes(hip_ctx, p, capi.ARITH_CERTIFIED)
    for d in range(2):
        assert np.array_equal(exact[d][0], cert[d][0]), "direction %d" % d
    assert np.array_equal(exact[2][0], cert[2][0]) and np.array_equal(exact[2][1], cert[2][1])
    print("redo fall-back 64x12x1030: certified %s flagged %s" % ([cert[d][1]["n_certified"] for d in range(2)], [cert[d][1]["n_flagged"] for d in range(2)]))


# ------------------------------------------------------------------------------------------------------ prologue
def _prologue_case(D, radius=5):
    import cases
    return cases.get_twoview("geodesic_masks", w=FILL_W, h=40, D=D, radius=radius)


def _fresh(case, p):
    with capi.Context(0) as c:
        _upload(c, case)
        c.set_option("strip", 8)
        return [_bits(m).copy() for m in c.twoview_compute(0, 1, p)]


def test_prologue_back_to_back_calls_on_one_context(hip_ctx):
    """One pair; 40 labels, then 24, then 40 with another window radius, one call behind the other with nothing but the
    calls' own waits in between: the side stream's tables and ranges of one call must not reach the kernels of another"""
    case = _prologue_case(40)
    ps = []
    for D, radius in ((40, 5), (24, 5), (40, 2)):
        zmin, zmax = synthetic.rectified_depth_range(FILL_W, D)
        ps.append(capi.params_twoview(min_depth=zmin, max_depth=zmax, num_depth_levels=D, window_radius=radius,
                                      weight_kind=capi.WEIGHT_GEODESIC))
    want = [_fresh(case, p) for p in ps]
    _upload(hip_ctx, case)
    with _Options(hip_ctx, strip=8):
        got = [[_bits(m).copy() for m in hip_ctx.twoview_compute(0, 1, p)] for p in ps]
    for k in range(3):
        for d in range(2):
            assert np.array_equal(got[k][d], want[k][d]), "call %d, map %d: %d depths differ from a fresh context's" % (k, d, (got[k][d] != want[k][d]).sum())


@pytest.mark.parametrize("budget", [32768, 1], ids=["one-band", "bands"])
def test_prologue_overlap_and_side_stream_settings(hip_ctx, budget):
    case = _prologue_case(40)
    p = _upload(hip_ctx, case)
    maps = {}
    for ov in (0, 1):
        for sw in (0, 1):
            with _Options(hip_ctx, strip=8, tv_overlap=ov, side_weights=sw, band_budget_mb=budget):
                maps[ov, sw] = [_bits(m).copy() for m in hip_ctx.twoview_compute(0, 1, p)]
    for key, m in maps.items():
        for d in range(2):
            assert np.array_equal(m[d], maps[0, 0][d]), "tv_overlap %d side_weights %d, map %d" % (key[0], key[1], d)
    import cases
    import oracle_ffi as O
    imgs, ocams, op = cases.oracle_inputs(case)
    dl = O.twoview_wta(imgs[0], imgs[1], ocams[0], ocams[1], op)
    dr = O.twoview_wta(imgs[1], imgs[0], ocams[1], ocams[0], op)
    cl, cr_ = O.twoview_cross_check(ocams[0], ocams[1], op, dl, dr)
    with _Options(hip_ctx, strip=8, band_budget_mb=budget):
        gl, gr = hip_ctx.twoview_compute(0, 1, p)
    _assert_depth(gl, cl, "left")
    _assert_depth(gr, cr_, "right")


def test_prologue_sad_on_the_dense_plan(hip_ctx):
    """cost_sad with sad_dense shares the dense plan's preparation: side stream on and off, the same bits"""
    case = _prologue_case(40)
    p = _upload(hip_ctx, case)
    maps = []
    for sw in (0, 1):
        with _Options(hip_ctx, cost=capi.COST_SAD, sad_dense=1, side_weights=sw):
            maps.append([_bits(m).copy() for m in hip_ctx.twoview_compute(0, 1, p)])
            assert hip_ctx.stats()["used_dense_path"]
    for d in range(2):
        assert np.array_equal(maps[0][d], maps[1][d]), "map %d" % d
