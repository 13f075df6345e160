"""Option "subpixel" (srh_subpixel.hip) on the GPU: against the CPU reference of tests/subpixel_ref.py, bit for
bit against a replay from the device's own planes, across every plan of the library, over bands, row ranges and odd shapes,
on the class scene, with the option off, and through srh_twoview_compute."""
import contextlib
import math
import struct
import subprocess

import numpy as np
import pytest

import cases
import oracle_ffi as O
import sad_ref as S
import subpixel_ref as SR
import test_gpu_host_api as HA
from stereoreconstruction_amd import capi
from test_gpu_wta_outputs import _decision_gap
from test_subpixel_ref import build_host_program

pytestmark = pytest.mark.gpu

DEFAULTS = dict(subpixel=0, wta_outputs=0, arith=capi.ARITH_DEFAULT, strip=1, tscan=1, fused=0, force_generic=0, list_rows=1,
                tv_overlap=1, cost=capi.COST_NCC, sad_dense=0, band_budget_mb=32768)
PLANES = ("delta", "neigh_xy", "cls")
DIRECTIONS = ((0, 1), (1, 0))


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


def _setup(ctx, case):
    cams, p = cases.hip_inputs(case)
    cases.upload_case(ctx, case, cams)
    return p


def _pass(ctx, ref, oth, p, y0=0, y1=0):
    """one refined WTA pass (the caller set the options) -> dict(depth, delta, neigh_xy, cls, win_xy, min_cost, stats)"""
    ctx.twoview_wta(ref, oth, p, y0, y1)
    out = dict(depth=ctx.download_depth(ref), stats=ctx.stats())
    out.update(ctx.subpixel(ref))
    w = ctx.wta_outputs(ref)
    out["win_xy"], out["min_cost"] = w["win_xy"], w["min_cost"]
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, want, tag, keys=PLANES + ("depth",), rows=None):
    for k in keys:
        a, b = _bits(got[k]), _bits(want[k])
        if rows is not None:
            a, b = a[rows[0]:rows[1]], b[rows[0]:rows[1]]
        assert np.array_equal(a, b), "%s: %s differs at %d places, first %s" % (tag, k, (a != b).sum(), np.argwhere(a != b)[:3].tolist())


_REFERENCE = {}


def _reference(name, case):
    """the CPU reference of both directions of a case, computed once: [(integer depth, oracle diagnostics, refined dict)]"""
    if name not in _REFERENCE:
        imgs, ocams, op = cases.oracle_inputs(case)
        _REFERENCE[name] = [SR.reference_pass(imgs, ocams, op, ref, oth) for ref, oth in DIRECTIONS]
    return _REFERENCE[name]


def _tol(*costs):
    """e = 1e-9 * max(1, |c|): the project's cost tolerance (device exp against libm's)"""
    return 1e-9 * max(1.0, *[abs(c) for c in costs])


# ---------------------------------------------------------------------------------------------- 1. against the reference
ORACLE_CASES = ["geodesic_r2", "adaptive_masks", "geodesic_verged_dist_masks", "adaptive_refractive", "geodesic_scaled"]


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_against_the_cpu_reference(hip_ctx, name):
    """Neighbours and classes equal, delta within 3e/D (numerator off by at most 2e, D by at most 4e, |cm - cp|/D <= 1), depth
    within 1e-9 relative.  Left out: a pixel whose winner already disagrees (the decision-gap rule of
    test_gpu_wta_outputs.py), or that the reference's own numbers put within that error of a class boundary: D <= 4e or
    ||delta| - 0.5| <= 3e/D.  At most 1 % of the WHITE pixels."""
    compare_with_the_cpu_reference(hip_ctx, name, cases.get_twoview(name))


def compare_with_the_cpu_reference(hip_ctx, name, case):
    """the comparison of test_against_the_cpu_reference on any case (tests/test_gpu_radii_twoview.py: other radii); `name`
    keys the shared reference and tags the messages -> per direction (pixels left out, class counts)"""
    p = _setup(hip_ctx, case)
    imgs, ocams, op = cases.oracle_inputs(case)
    reference = _reference(name, case)
    figures = []
    for k, (ref, oth) in enumerate(DIRECTIONS):
        integer, diag, want = reference[k]
        with _options(hip_ctx, subpixel=1, wta_outputs=3):
            got = _pass(hip_ctx, ref, oth, p)
        white = case["views"][ref][1] == 1
        left_out = 0
        keep = np.ones(white.shape, bool)
        for y, x in np.argwhere(white):
            c0 = diag["min_cost"][y, x]
            # (the winner, its cost and the ratio test's verdict: the refinement never changes whether a depth is finite)
            same_winner = (got["win_xy"][y, x] == diag["win_xy"][y, x]).all() and \
                (got["min_cost"][y, x] == c0 or abs(got["min_cost"][y, x] - c0) <= _tol(c0)) and \
                math.isfinite(got["depth"][y, x]) == math.isfinite(integer[y, x])
            if not same_winner:
                gap = _decision_gap(imgs, ocams, op, ref, oth, int(x), int(y))
                assert gap <= 1e-7, "%s %d>%d (%d,%d): winner disagrees, no decision within 1e-7 of flipping (gap %g)" % (name, ref, oth, x, y, gap)
                keep[y, x] = False
                continue
            tag = "%s %d>%d (%d,%d)" % (name, ref, oth, x, y)
            assert (got["neigh_xy"][y, x] == want["neigh_xy"][y, x]).all(), "%s: neighbours %s / %s" % (tag, got["neigh_xy"][y, x], want["neigh_xy"][y, x])
            if want["cls"][y, x] >= SR.FLAT:
                cm, cp, D = want["cm"][y, x], want["cp"][y, x], want["D"][y, x]
                e = _tol(cm, c0, cp)
                if D <= 4 * e or abs(abs(0.5 * (cm - cp) / D) - 0.5) <= 3 * e / D:
                    keep[y, x] = False
                    continue
                if want["cls"][y, x] == SR.REFINED:
                    assert abs(got["delta"][y, x] - want["delta"][y, x]) <= 3 * e / D, "%s: delta %r / %r, D %r" % (tag, got["delta"][y, x], want["delta"][y, x], D)
            assert got["cls"][y, x] == want["cls"][y, x], "%s: class %d / %d" % (tag, got["cls"][y, x], want["cls"][y, x])
        left_out = int((white & ~keep).sum())
        print("%s %d>%d: %d of %d WHITE pixels left out, classes %s" % (name, ref, oth, left_out, white.sum(), np.bincount(got["cls"].ravel(), minlength=5)))
        assert left_out <= 0.01 * white.sum()
        ok, msg, _ = cases.compare_depth(np.where(keep, got["depth"], 0.0), np.where(keep, want["depth"], 0.0), 1e-9)
        assert ok, "%s %d>%d: %s" % (name, ref, oth, msg)
        assert (got["cls"][~white] == SR.NONE).all() and (got["neigh_xy"][~white] == -1).all() and (got["delta"][~white] == 0).all()
        assert (got["delta"][got["cls"] != SR.REFINED] == 0).all()
        figures.append((left_out, np.bincount(got["cls"].ravel(), minlength=5)))
    return figures


# ---------------------------------------------------------------------------------------------- 2. bit-exact replay
def _replay(ctx, case, p, ref, oth, got, integer, kind=capi.COST_NCC, rows=None):
    """The definition replayed from the device's own planes, independent of the host's libm: the neighbours are the rule
    applied to the oracle's curves and the device's winners and integer depths; cm, c0, cp fetched with
    srh_twoview_pair_costs give delta and the class in Python floats, bit for bit; c0 is min_cost's bits; the oracle's
    triangulation at the device's delta gives the depth within 1e-9."""
    imgs, ocams, op = cases.oracle_inputs(case)
    h, w = integer.shape
    y0, y1 = rows if rows is not None else (0, h)
    white = case["views"][ref][1] == 1
    pairs, where = [], []
    for y in range(y0, y1):
        for x in range(w):
            tag = "%d>%d (%d,%d)" % (ref, oth, x, y)
            z0 = float(integer[y, x])
            win = tuple(int(v) for v in got["win_xy"][y, x])
            if not white[y, x] or win[0] < 0 or not math.isfinite(z0):
                assert got["cls"][y, x] == SR.NONE and (got["neigh_xy"][y, x] == -1).all() and got["delta"][y, x] == 0, tag
                assert S.same_bits(got["depth"][y, x:x + 1], integer[y, x:x + 1]), tag
                continue
            curve = O.epipolar_curve(ocams[ref], ocams[oth], imgs[oth], op, False, x, y)
            cset = set((int(a), int(b)) for a, b in curve)
            rsrc, rdir = SR.unproject(ocams[ref], (x + 0.5) / op.image_scale, (y + 0.5) / op.image_scale)
            nm, npl = SR.neighbours(cset, win, z0, lambda q: SR.depth_at(ocams[ref], ocams[oth], op, rsrc, rdir, q[0] + 0.5, q[1] + 0.5))
            want = list(nm or (-1, -1)) + list(npl or (-1, -1))
            assert got["neigh_xy"][y, x].tolist() == want, "%s: neighbours %s, the rule gives %s" % (tag, got["neigh_xy"][y, x], want)
            if nm is None or npl is None:
                assert got["cls"][y, x] == SR.NO_NEIGHBOUR and got["delta"][y, x] == 0, tag
                assert S.same_bits(got["depth"][y, x:x + 1], integer[y, x:x + 1]), tag
                continue
            pairs += [(x, y) + nm, (x, y) + win, (x, y) + npl]
            where.append((x, y, win, nm, npl, rsrc, rdir))
    if not pairs:                                                  # (a one-row view: sample() has no valid tap, no pixel has a winner)
        return np.bincount(got["cls"].ravel(), minlength=5)
    costs = ctx.twoview_pair_costs(ref, oth, p, np.array(pairs, np.int32), kind).reshape(-1, 3)
    for (x, y, win, nm, npl, rsrc, rdir), (cm, c0, cp) in zip(where, costs):
        tag = "%d>%d (%d,%d)" % (ref, oth, x, y)
        assert S.same_bits(got["min_cost"][y, x:x + 1], np.array([c0])), tag
        k, delta, _ = SR.classify(float(cm), float(c0), float(cp))
        assert got["cls"][y, x] == k, "%s: class %d, the replay gives %d" % (tag, got["cls"][y, x], k)
        assert S.same_bits(got["delta"][y, x:x + 1], np.array([delta])), "%s: delta %r, the replay gives %r" % (tag, got["delta"][y, x], delta)
        if k == SR.REFINED and delta != 0:
            qx, qy = SR.refined_position(win, nm, npl, delta)
            z = SR.depth_at(ocams[ref], ocams[oth], op, rsrc, rdir, qx, qy)
            assert abs(got["depth"][y, x] - z) <= 1e-9 * max(1.0, abs(z)), "%s: depth %r, the oracle's triangulation %r" % (tag, got["depth"][y, x], z)
        else:
            assert S.same_bits(got["depth"][y, x:x + 1], integer[y, x:x + 1]), tag
    return np.bincount(got["cls"].ravel(), minlength=5)


def _integer_and_refined(ctx, p, ref, oth, y0=0, y1=0, **opts):
    with _options(ctx, **opts):
        ctx.twoview_wta(ref, oth, p, y0, y1)
        integer = ctx.download_depth(ref)
    with _options(ctx, subpixel=1, wta_outputs=3, **opts):
        got = _pass(ctx, ref, oth, p, y0, y1)
    return integer, got


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_replay_from_the_devices_own_planes(hip_ctx, name):
    case = cases.get_twoview(name)
    p = _setup(hip_ctx, case)
    for ref, oth in DIRECTIONS:
        integer, got = _integer_and_refined(hip_ctx, p, ref, oth)
        counts = _replay(hip_ctx, case, p, ref, oth, got, integer)
        assert counts[SR.REFINED] > 0 and counts[SR.NO_NEIGHBOUR] > 0


def test_replay_under_sad(hip_ctx):
    case = cases.get_twoview("adaptive_masks")
    p = _setup(hip_ctx, case)
    for ref, oth in DIRECTIONS:
        integer, got = _integer_and_refined(hip_ctx, p, ref, oth, cost=capi.COST_SAD)
        counts = _replay(hip_ctx, case, p, ref, oth, got, integer, kind=capi.COST_SAD)
        assert counts[SR.REFINED] > 0


# ---------------------------------------------------------------------------------------------- 3. every plan, the same bits
def _dense(st):
    return st["used_dense_path"]


NCC_PLANS = [
    ("defaults", dict(), _dense),
    ("strip 0", dict(strip=0), lambda st: _dense(st) and not st["used_strip_kernel"]),
    ("strip 0 tscan 0", dict(strip=0, tscan=0), lambda st: _dense(st) and not st["used_strip_kernel"] and st["scan_tiles_template"] == 0),
    ("strip 1 tscan 0", dict(tscan=0), lambda st: _dense(st) and st["scan_tiles_template"] == 0),
    ("arith 0", dict(arith=0), lambda st: _dense(st) and st["n_certified"] == 0),
    ("arith 3", dict(arith=3), _dense),
    ("fused", dict(fused=1), lambda st: st["used_fused_kernel"]),
    ("row-run lists", dict(force_generic=1, list_rows=1), lambda st: not _dense(st)),
    ("list order", dict(force_generic=1, list_rows=0), lambda st: not _dense(st)),
]
SAD_PLANS = [
    ("sad lists", dict(cost=capi.COST_SAD, sad_dense=0), lambda st: not _dense(st)),
    ("sad dense", dict(cost=capi.COST_SAD, sad_dense=1), _dense),
    ("sad list order", dict(cost=capi.COST_SAD, list_rows=0), lambda st: not _dense(st)),
]


@pytest.mark.parametrize("name", ["geodesic_rect", "geodesic_r2"])
def test_every_plan_gives_the_walk_kernels_bits(hip_ctx, name):
    case = cases.get_twoview(name)
    p = _setup(hip_ctx, case)
    for plans, base in ((NCC_PLANS, dict()), (SAD_PLANS, dict(cost=capi.COST_SAD))):
        with _options(hip_ctx, subpixel=1, wta_outputs=3, force_generic=2, arith=0, **base):
            want = [_pass(hip_ctx, ref, oth, p) for ref, oth in DIRECTIONS]
        for w in want:
            assert not w["stats"]["used_dense_path"] and (w["cls"] == SR.REFINED).any()
        for tag, opts, ran in plans:
            with _options(hip_ctx, subpixel=1, wta_outputs=3, **opts):
                for k, (ref, oth) in enumerate(DIRECTIONS):
                    got = _pass(hip_ctx, ref, oth, p)
                    assert ran(got["stats"]), "%s %s: the intended plan did not run: %s" % (name, tag, got["stats"])
                    _same(got, want[k], "%s %s %d>%d" % (name, tag, ref, oth))


@pytest.mark.parametrize("name,over,opts", [("geodesic_rect", dict(), dict()), ("geodesic_rect", dict(), dict(strip=0)),
                                            ("geodesic_verged_dist_masks", dict(radius=5), dict()),
                                            ("geodesic_verged_dist_masks", dict(radius=5), dict(list_rows=0)),
                                            ("adaptive_rect", dict(), dict(force_generic=2))])
def test_bands_give_the_bits_of_one_band(hip_ctx, name, over, opts):
    case = cases.get_twoview(name, **over)
    p = _setup(hip_ctx, case)
    h, w = case["views"][0][0].shape[:2]
    taps = (2 * p.window_radius + 1) ** 2
    assert math.ceil(h / ((1 << 20) // (taps * 8 * w))) >= 3     # 1 MB holds so few rows of windows that the pass takes 3 bands
    for ref, oth in DIRECTIONS:
        with _options(hip_ctx, subpixel=1, wta_outputs=3, **opts):
            one = _pass(hip_ctx, ref, oth, p)
        with _options(hip_ctx, subpixel=1, wta_outputs=3, band_budget_mb=1, **opts):
            many = _pass(hip_ctx, ref, oth, p)
        assert (one["cls"] == SR.REFINED).any()
        _same(many, one, "%s %s banded %d>%d" % (name, opts, ref, oth))


@pytest.mark.parametrize("name,opts", [("geodesic_rect", dict()), ("geodesic_verged_dist_masks", dict()), ("adaptive_rect", dict(force_generic=2))])
def test_a_row_range_refines_its_rows_only(hip_ctx, name, opts):
    case = cases.get_twoview(name)
    p = _setup(hip_ctx, case)
    with _options(hip_ctx, subpixel=1, wta_outputs=3, **opts):
        full = _pass(hip_ctx, 0, 1, p)
    _setup(hip_ctx, case)                                          # freshly uploaded views: NaN depth, no planes
    with _options(hip_ctx, subpixel=1, wta_outputs=3, **opts):
        part = _pass(hip_ctx, 0, 1, p, 7, 19)
    _same(part, full, "%s rows [7,19)" % name, rows=(7, 19))
    for rows in ((0, 7), (19, None)):
        sl = slice(*rows)
        assert np.isnan(part["depth"][sl]).all() and (part["cls"][sl] == SR.NONE).all()
        assert (part["neigh_xy"][sl] == -1).all() and (part["delta"][sl] == 0).all()
    # a second range on top: the first one's rows keep what they hold
    with _options(hip_ctx, subpixel=1, wta_outputs=3, **opts):
        more = _pass(hip_ctx, 0, 1, p, 19, 30)
    _same(more, full, "%s rows [7,30)" % name, rows=(7, 30))


@pytest.mark.parametrize("w,h", [(31, 12), (33, 12), (48, 12), (40, 1)])
@pytest.mark.parametrize("opts", [dict(), dict(force_generic=1)], ids=["dense", "lists"])
def test_tile_tails_and_a_one_row_view(hip_ctx, w, h, opts):
    """widths around the 32-pixel window tile and a single row, replayed exactly; winners occur in columns 0 and w - 1 of
    the other view"""
    case = cases.get_twoview("geodesic_r2", w=w, h=h, D=12)
    p = _setup(hip_ctx, case)
    cols = set()
    for ref, oth in DIRECTIONS:
        integer, got = _integer_and_refined(hip_ctx, p, ref, oth, **opts)
        _replay(hip_ctx, case, p, ref, oth, got, integer)
        cols |= set(got["win_xy"][..., 0][np.isfinite(integer)].tolist())
    if h > 1:
        assert 0 in cols and w - 1 in cols, sorted(cols)


# ---------------------------------------------------------------------------------------------- 4. the class scene
def test_every_class_occurs_and_the_counts_are_the_infos(hip_ctx):
    """slanted plane, 64x40, D = 16, radius 2, AdaptiveWeight, 40 % of the rows flat: on the CPU reference pass 1>0 holds
    every class (NO_NEIGHBOUR 389, FLAT 603, OUTSIDE 9, REFINED 1228, 4 of them with delta == 0)"""
    case = SR.slanted_case(weight_kind=0, radius=2, flat_frac=0.4)
    p = _setup(hip_ctx, case)
    seen = np.zeros(5, np.int64)
    zero = 0
    for ref, oth in DIRECTIONS:
        integer, got = _integer_and_refined(hip_ctx, p, ref, oth)
        info = hip_ctx.subpixel_info(ref)
        counts = np.bincount(got["cls"].ravel(), minlength=5)
        print("class scene %d>%d: %s, delta == 0: %d" % (ref, oth, dict(zip(SR.CLASS_NAMES, counts.tolist())), ((got["cls"] == SR.REFINED) & (got["delta"] == 0)).sum()))
        assert info["n_class"] == counts.tolist()
        assert info["n_moved"] == int(((got["cls"] == SR.REFINED) & (got["delta"] != 0)).sum())
        assert np.array_equal(_replay(hip_ctx, case, p, ref, oth, got, integer), counts)
        seen += counts
        zero += int(((got["cls"] == SR.REFINED) & (got["delta"] == 0)).sum())
    assert (seen > 0).all(), dict(zip(SR.CLASS_NAMES, seen.tolist()))
    assert zero > 0


# ---------------------------------------------------------------------------------------------- 5. option off
def _invalid(fn, *a):
    with pytest.raises(capi.StereoHipError) as e:
        fn(*a)
    assert e.value.code == capi.SRH_E_INVALID, e.value


def test_option_off_changes_nothing_and_holds_nothing(hip_ctx):
    case = cases.get_twoview("adaptive_masks")
    with capi.Context(0) as fresh:                                  # a context that never saw the option
        p = _setup(fresh, case)
        before = fresh.twoview_compute(0, 1, p)
        for fn in (fresh.subpixel, fresh.subpixel_device, fresh.subpixel_info):
            _invalid(fn, 0)
        assert fresh.wta_outputs_state(0) == (0, -1)
    p = _setup(hip_ctx, case)
    for bad in (2, -1):
        _invalid(hip_ctx.set_option, "subpixel", bad)
    with _options(hip_ctx, subpixel=1):
        on = hip_ctx.twoview_compute(0, 1, p)
        assert hip_ctx.wta_outputs_state(0) == (0, -1)             # what "wta_outputs" asked for: nothing
        _invalid(hip_ctx.wta_outputs, 0)
        assert all(hip_ctx.subpixel_device(0)) and (hip_ctx.subpixel(0)["cls"] == SR.REFINED).any()
    with _options(hip_ctx, subpixel=1, wta_outputs=1):
        hip_ctx.twoview_wta(0, 1, p)
        assert hip_ctx.wta_outputs_state(0) == (1, 1) and sorted(hip_ctx.wta_outputs(0)) == ["runner_xy", "win_xy"]
    off = hip_ctx.twoview_compute(0, 1, p)
    for k in range(2):
        assert S.same_bits(off[k], before[k])
        assert not S.same_bits(on[k], before[k])
        for fn in (hip_ctx.subpixel, hip_ctx.subpixel_device, hip_ctx.subpixel_info):
            _invalid(fn, k)
    # uploaded since: nothing held
    with _options(hip_ctx, subpixel=1):
        hip_ctx.twoview_wta(0, 1, p)
        hip_ctx.subpixel(0)
        _setup(hip_ctx, case)
        _invalid(hip_ctx.subpixel, 0)


# ---------------------------------------------------------------------------------------------- 6. srh_twoview_compute
@pytest.mark.parametrize("name", ["geodesic_rect", "geodesic_verged_dist_masks"])
@pytest.mark.parametrize("overlap", [1, 0])
def test_compute_is_two_refined_passes_and_the_cross_check(hip_ctx, name, overlap):
    case = cases.get_twoview(name)
    p = _setup(hip_ctx, case)
    with _options(hip_ctx, subpixel=1):
        planes = []
        for ref, oth in DIRECTIONS:
            hip_ctx.twoview_wta(ref, oth, p)
            planes.append(hip_ctx.subpixel(ref))
        hip_ctx.twoview_cross_check(0, 1, p)
        want = [hip_ctx.download_depth(k) for k in range(2)]
    _setup(hip_ctx, case)
    with _options(hip_ctx, subpixel=1, tv_overlap=overlap):
        got = hip_ctx.twoview_compute(0, 1, p)
        for k in range(2):
            assert S.same_bits(got[k], want[k]), "%s slot %d" % (name, k)
            _same(hip_ctx.subpixel(k), planes[k], "%s compute slot %d" % (name, k), keys=PLANES)


def test_the_label_volume_stages_ignore_the_option(hip_ctx):
    case = cases.get_twoview("geodesic_r2")
    p = _setup(hip_ctx, case)
    for run in (hip_ctx.twoview_compute_mrf, hip_ctx.twoview_compute_sgm):
        off = run(0, 1, p)
        with _options(hip_ctx, subpixel=1):
            on = run(0, 1, p)
            _invalid(hip_ctx.subpixel, 0)
        for k in range(2):
            assert S.same_bits(on[k], off[k])


# ---------------------------------------------------------------------------------------------- 7. host class
def _read_host_output(path, w, h):
    raw = open(path, "rb").read()
    n = w * h
    maps = [np.frombuffer(raw, np.float64, n, k * n * 8).reshape(h, w) for k in range(2)]
    counts = struct.unpack_from("<2i", raw, 2 * n * 8)
    off = 2 * n * 8 + 8
    deltas = []
    for cnt in counts:
        deltas.append(np.frombuffer(raw, np.float64, cnt, off))
        off += cnt * 8
    assert off == len(raw)
    return maps, deltas


def test_host_class_with_subpixel_equals_the_c_abi_path(hip_ctx, tmp_path):
    exe = build_host_program(tmp_path)
    case = cases.get_twoview("geodesic_masks", w=48, h=36)
    w, h = 48, 36
    inp = str(tmp_path / "in.bin")
    HA._write_input(inp, case, True)
    p = _setup(hip_ctx, case)
    want = {}
    for on in (1, 0):
        with _options(hip_ctx, subpixel=on):
            want[on] = (hip_ctx.twoview_compute(0, 1, p), [hip_ctx.subpixel(k)["delta"] for k in range(2)] if on else None)
    assert not S.same_bits(want[1][0][0], want[0][0][0])
    for on in (1, 0):
        outp = str(tmp_path / ("out%d.bin" % on))
        subprocess.check_call([exe, inp, outp, str(on)])
        maps, deltas = _read_host_output(outp, w, h)
        for k in range(2):
            assert S.same_bits(maps[k], want[on][0][k]), (on, k)
            if on:
                assert S.same_bits(deltas[k], want[1][1][k].reshape(-1)), k
            else:
                assert deltas[k].size == 0
    # under the MRF stage no scan makes the maps: empty vectors
    outp = str(tmp_path / "out_mrf.bin")
    subprocess.check_call([exe, inp, outp, "1", "mrf"])
    assert all(d.size == 0 for d in _read_host_output(outp, w, h)[1])


# ---------------------------------------------------------------------------------------------- quality
@pytest.mark.parametrize("weight_kind,radius", [(capi.WEIGHT_GEODESIC, 5), (capi.WEIGHT_ADAPTIVE, 2)])
def test_refined_disparities_are_closer_to_the_truth(hip_ctx, weight_kind, radius):
    """The slanted plane with an analytic texture (tests/subpixel_ref.py): over the REFINED pixels the median absolute
    disparity error and the inlier RMS are lower for the refined map than for the integer map of the same run, and both are
    the CPU reference's values to the parity tolerance: 1e-9 relative in depth is below 1e-7 px here."""
    case = SR.slanted_case(weight_kind=weight_kind, radius=radius)
    p = _setup(hip_ctx, case)
    reference = _reference("slanted %d %d" % (weight_kind, radius), case)
    for k, (ref, oth) in enumerate(DIRECTIONS):
        integer, got = _integer_and_refined(hip_ctx, p, ref, oth)
        e = SR.disparity_errors(integer, got["depth"], got["cls"], 64, ref)
        cpu = SR.disparity_errors(reference[k][0], reference[k][2]["depth"], reference[k][2]["cls"], 64, ref)
        print("slanted, weights %d radius %d, %d>%d: device %s, CPU reference %s" % (weight_kind, radius, ref, oth, e, cpu))
        assert e["median_sub"] < e["median_int"] and e["rms_sub"] < e["rms_int"]
        assert e["n"] == cpu["n"]
        for key in ("median_int", "median_sub", "rms_int", "rms_sub"):
            assert abs(e[key] - cpu[key]) <= 1e-7, key
