"""srh_mvs_view_subpixel (srh_mvs_subpixel.hip) on the GPU: against the definition of tests/mvs_subpixel_ref.py
applied to the device's own map from before the stage -- after the WTA, the semi-global stage, TRW-S and on uploaded maps --
the narrowed search against the exhaustive one, odd shapes, radii and neighbour counts, row bands, the stage not called,
the cross-check behind it, the host class, and the quality scene."""
import contextlib
import subprocess

import numpy as np
import pytest

import cases
import mvs_subpixel_ref as MR
import oracle_ffi as O
import test_gpu_host_api as HA
from stereoreconstruction_amd import capi
from test_mvs_subpixel_ref import SMALL, build_host_program, plane_reference, small_geodesic

pytestmark = pytest.mark.gpu

DEFAULTS = dict(mvs_subpixel_search=0, band_budget_mb=32768, debug_alloc_limit_mb=0, force_generic=0)
PLANES = ("win", "neigh_xy", "cls", "delta")
CASES = [("mvs_geodesic", SMALL), ("mvs_adaptive", {}), ("mvs_distorted", {}), ("mvs_refractive", {}), ("mvs_scaled", {}),
         ("mvs_mixed_sizes", {}), ("mvs_five_views", {})]


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


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, want, tag, keys=PLANES + ("depth",)):
    for k in keys:
        a, b = _bits(got[k]), _bits(want[k])
        assert np.array_equal(a, b), "%s: %s differs at %d places, first %s" % (tag, k, (a != b).sum(), np.argwhere(a != b)[:3].tolist())


def _setup(ctx, case):
    imgs, ocams, op = cases.oracle_inputs(case)
    cams, p = cases.hip_inputs(case)
    cases.upload_case(ctx, case, cams)
    return imgs, ocams, op, O.mvs_neighbours(ocams, op), p


def _stage(ctx, v, neigh, p, before=None, **opts):
    """the stage on the slot's map (or on `before`, uploaded first) -> the planes, the info and the refined map"""
    if before is not None:
        ctx.upload_depth(v, before)
    with _options(ctx, **opts):
        got = ctx.mvs_view_subpixel(v, neigh, p, want_planes=True)
    got["depth"] = ctx.download_depth(v)
    return got


def _tol(*costs):
    """e = 1e-9 * max(1, |c|): the project's cost tolerance (tests/test_gpu_subpixel.py)"""
    return 1e-9 * max(1.0, *[abs(c) for c in costs])


def _check_info(got, before, mask, exhaustive=False):
    counts = np.bincount(got["cls"].ravel(), minlength=6)
    assert got["n_class"] == counts.tolist()
    assert got["n_moved"] == int(((got["cls"] == MR.REFINED) & (got["delta"] != 0)).sum())
    # the narrowed search hands over exactly the pixels that have no winner at all: its bound holds
    assert got["n_fallback"] == (0 if exhaustive else int(counts[MR.NO_WINNER]))
    none = (mask != 1) | ~np.isfinite(before) | ~(before > 0)
    assert np.array_equal(got["cls"] == MR.NONE, none)
    assert (got["win"][got["cls"] == MR.NONE] == -1).all() and (got["win"][got["cls"] == MR.NO_WINNER] == -1).all()
    assert (got["delta"][got["cls"] != MR.REFINED] == 0).all()
    kept = ~((got["cls"] == MR.REFINED) & (got["delta"] != 0))
    assert np.array_equal(_bits(got["depth"])[kept], _bits(before)[kept]), "a pixel that is not moved keeps its depth's bits"
    return counts


def _compare(got, want, before, mask, tag):
    """Winner, n-, n+ and class exact, delta within 3e/D, depth within 1e-9 relative (the rule of tests/test_gpu_subpixel.py).
    Left out: a pixel the reference's own numbers put within the cost tolerance of a class boundary: |D| <= 4e (here the
    winner need not hold the maximum: D may be far below 0, which is FLAT for certain) or, for D > 0, ||delta| - 0.5| <= 3e/D; at most 1 % of the view's pixels with a peak.  -> pixels left out"""
    assert np.array_equal(got["win"], want["win"]), "%s: winners differ at %s" % (tag, np.argwhere((got["win"] != want["win"]).any(-1))[:3].tolist())
    assert np.array_equal(got["neigh_xy"], want["neigh_xy"]), "%s: neighbours differ at %s" % (tag, np.argwhere((got["neigh_xy"] != want["neigh_xy"]).any(-1))[:3].tolist())
    keep = np.ones(before.shape, bool)
    for y, x in np.argwhere(want["cls"] >= MR.FLAT):
        if want["cls"][y, x] == MR.NO_WINNER:
            continue
        cm, c0, cp, D = want["cm"][y, x], want["c0"][y, x], want["cp"][y, x], want["D"][y, x]
        e = _tol(cm, c0, cp)
        if abs(D) <= 4 * e or (D > 0 and abs(abs(0.5 * (cp - cm) / D) - 0.5) <= 3 * e / D):
            keep[y, x] = False
            continue
        if want["cls"][y, x] == MR.REFINED:
            assert abs(got["delta"][y, x] - want["delta"][y, x]) <= 3 * e / D, "%s (%d,%d): delta %r / %r, D %r" % (tag, x, y, got["delta"][y, x], want["delta"][y, x], D)
    assert np.array_equal(got["cls"][keep], want["cls"][keep]), "%s: classes differ at %s" % (tag, np.argwhere(keep & (got["cls"] != want["cls"]))[:3].tolist())
    peaks = int((np.isfinite(before) & (before > 0) & (mask == 1)).sum())
    left_out = int((~keep).sum())
    assert left_out <= 0.01 * peaks, "%s: %d of %d pixels left out" % (tag, left_out, peaks)
    ok, msg, _ = cases.compare_depth(np.where(keep, got["depth"], 0.0), np.where(keep, want["depth"], 0.0), 1e-9)
    assert ok, "%s: %s" % (tag, msg)
    return left_out


# ---------------------------------------------------------------------------------------------- 1. the definition, both searches
@pytest.mark.parametrize("name,over", CASES, ids=[c[0] for c in CASES])
def test_against_the_definition_and_the_exhaustive_search(hip_ctx, name, over):
    """every view: mvs_initial_estimate, the map downloaded, the stage; the definition applied to that device map.  Then the
    same map once more under "mvs_subpixel_search" = 1: identical planes and depth bits, and no pixel fell back"""
    case = cases.get_mvs(name, **over)
    imgs, ocams, op, neigh, p = _setup(hip_ctx, case)
    for v in range(len(ocams)):
        tag = "%s view %d" % (name, v)
        mask = case["views"][v][1]
        hip_ctx.mvs_initial_estimate(v, neigh[v], p)
        before = hip_ctx.download_depth(v)
        got = _stage(hip_ctx, v, neigh[v], p)
        counts = _check_info(got, before, mask)
        want = MR.refine_view(imgs, ocams, op, v, neigh[v], before)
        left_out = _compare(got, want, before, mask, tag)
        print("%s: %s, %d left out, %d fell back" % (tag, dict(zip(MR.CLASS_NAMES, counts.tolist())), left_out, got["n_fallback"]))
        assert counts[MR.REFINED] > 0 and counts[MR.NO_NEIGHBOUR] > 0 and counts[MR.NO_WINNER] == 0
        assert counts[MR.FLAT] == 0 and counts[MR.OUTSIDE] == 0          # (the WTA's winner holds the maximum)
        law = _stage(hip_ctx, v, neigh[v], p, before=before, mvs_subpixel_search=1)
        _check_info(law, before, mask, exhaustive=True)
        _same(got, law, tag + " narrowed / exhaustive")


# ---------------------------------------------------------------------------------------------- 2. other estimators
@pytest.mark.parametrize("stage", ["sgm", "mrf"])
def test_after_the_label_stages(hip_ctx, stage):
    """the definition is applied to the device's own pre-stage map, so the unpinned solvers do not enter; they pick peaks that
    are not the best one: FLAT and OUTSIDE occur"""
    name = "mvs_geodesic" if stage == "sgm" else "mvs_adaptive"
    case = cases.get_mvs(name, **SMALL)
    imgs, ocams, op, neigh, p = _setup(hip_ctx, case)
    seen = np.zeros(6, np.int64)
    for v in range(3):
        (hip_ctx.mvs_initial_estimate_sgm if stage == "sgm" else hip_ctx.mvs_initial_estimate_mrf)(v, neigh[v], p)
        before = hip_ctx.download_depth(v)
        got = _stage(hip_ctx, v, neigh[v], p)
        seen += _check_info(got, before, case["views"][v][1])
        _compare(got, MR.refine_view(imgs, ocams, op, v, neigh[v], before), before, case["views"][v][1], "%s %s view %d" % (name, stage, v))
        law = _stage(hip_ctx, v, neigh[v], p, before=before, mvs_subpixel_search=1)
        _same(got, law, "%s %s view %d narrowed / exhaustive" % (name, stage, v))
    print("%s after %s: %s" % (name, stage, dict(zip(MR.CLASS_NAMES, seen.tolist()))))
    assert seen[MR.FLAT] > 0 and seen[MR.OUTSIDE] > 0 and seen[MR.REFINED] > 0 and seen[MR.NO_WINNER] == 0


# ---------------------------------------------------------------------------------------------- 3. uploaded maps
def test_uploaded_maps(hip_ctx):
    """through srh_view_depth_upload: every pixel's second-best peak (NO_NEIGHBOUR 119, FLAT 12, OUTSIDE 37, REFINED 240 on the
    CPU) and the WTA map times (1 + 2^-40): NO_WINNER wherever there is a peak, every one of them through the fallback"""
    imgs, ocams, op, neigh, depth, peaks = small_geodesic()
    case = cases.get_mvs("mvs_geodesic", **SMALL)
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    mask = case["views"][0][1]
    second, replaced = MR.peak_map(peaks, 1)
    got = _stage(hip_ctx, 0, neigh[0], p, before=second)
    counts = _check_info(got, second, mask)
    want = MR.refine_view(imgs, ocams, op, 0, neigh[0], second)
    _compare(got, want, second, mask, "second-best peaks")
    for k in (MR.NO_NEIGHBOUR, MR.FLAT, MR.OUTSIDE, MR.REFINED):
        assert counts[k] > 0, MR.CLASS_NAMES[k]
    assert counts[MR.NO_WINNER] == 0
    _same(got, _stage(hip_ctx, 0, neigh[0], p, before=second, mvs_subpixel_search=1), "second-best peaks narrowed / exhaustive")
    off = depth * (1.0 + 2.0 ** -40)
    has = np.isfinite(depth) & (depth > 0) & (mask == 1)
    for search in (0, 1):
        got = _stage(hip_ctx, 0, neigh[0], p, before=off, mvs_subpixel_search=search)
        _check_info(got, off, mask, exhaustive=bool(search))
        assert (got["cls"][has] == MR.NO_WINNER).all() and got["n_class"][MR.NO_WINNER] == has.sum()
        assert np.array_equal(_bits(got["depth"]), _bits(off)) and (got["neigh_xy"] == -1).all()
    # a second call on a refined map: (nearly) no winner, (nearly) nothing moves
    first = _stage(hip_ctx, 0, neigh[0], p, before=depth)
    again = _stage(hip_ctx, 0, neigh[0], p)
    moved = (first["cls"] == MR.REFINED) & (first["delta"] != 0)
    assert (again["cls"][moved] == MR.NO_WINNER).mean() > 0.95


# ---------------------------------------------------------------------------------------------- 4. shapes, radii, neighbours
@pytest.mark.parametrize("over,nneigh", [(dict(w=31, h=12), 2), (dict(w=33, h=12), 2), (dict(w=40, h=1), 2), (dict(w=40, h=28), 1), (dict(w=40, h=28), 0),
                                         (dict(w=40, h=28, radius=1), 2), (dict(w=40, h=28, radius=3), 2), (dict(w=33, h=20, radius=3, weight_kind=0), 2)],
                         ids=["w31", "w33", "one-row", "nneigh1", "nneigh0", "r1", "r3", "r3-adaptive"])
def test_small_shapes_radii_and_neighbour_counts(hip_ctx, over, nneigh):
    case = cases.get_mvs("mvs_geodesic", D=12, nviews=3, **over)
    imgs, ocams, op, neigh, p = _setup(hip_ctx, case)
    assert p.window_radius == over.get("radius", 2)
    for v in (0, 1):
        nb = neigh[v][:nneigh]
        mask = case["views"][v][1]
        hip_ctx.mvs_initial_estimate(v, neigh[v], p)                   # (the map of the full neighbour list)
        before = hip_ctx.download_depth(v)
        got = _stage(hip_ctx, v, nb, p)
        counts = _check_info(got, before, mask)
        want = MR.refine_view(imgs, ocams, op, v, nb, before)
        _compare(got, want, before, mask, "%s nneigh %d view %d" % (over, nneigh, v))
        _same(got, _stage(hip_ctx, v, nb, p, before=before, mvs_subpixel_search=1), "%s view %d narrowed / exhaustive" % (over, v))
        if nneigh == 0:
            assert counts[MR.NONE] + counts[MR.NO_WINNER] == before.size
        elif nneigh == 1 and over["h"] > 1:
            assert counts[MR.NO_WINNER] > 0 and counts[MR.REFINED] > 0  # (the depths the other neighbour gave)


def test_bad_arguments(hip_ctx):
    case = cases.get_mvs("mvs_geodesic", **SMALL)
    _, _, _, neigh, p = _setup(hip_ctx, case)
    for args in ((17, [1, 2]), (0, [0, 1]), (0, [1, 17]), (0, list(range(1, 10))), (-1, [1])):
        with pytest.raises(capi.StereoHipError) as e:
            hip_ctx.mvs_view_subpixel(args[0], args[1], p)
        assert e.value.code == capi.SRH_E_INVALID, args
    for bad in (2, -1):
        with pytest.raises(capi.StereoHipError) as e:
            hip_ctx.set_option("mvs_subpixel_search", bad)
        assert e.value.code == capi.SRH_E_INVALID


# ---------------------------------------------------------------------------------------------- 5. row bands
def test_bands_give_the_bits_of_one_band(hip_ctx):
    """radius 5 windows of a 56-pixel row are 61 952 bytes: a 1 MB budget holds 19 rows, the 40 rows take 3 bands"""
    case = cases.get_mvs("mvs_geodesic", nviews=3, radius=5)
    _, _, _, neigh, p = _setup(hip_ctx, case)
    h, w = case["views"][0][0].shape[:2]
    assert -(-h // ((1 << 20) // (121 * 8 * w))) >= 3
    hip_ctx.mvs_initial_estimate(0, neigh[0], p)
    before = hip_ctx.download_depth(0)
    one = _stage(hip_ctx, 0, neigh[0], p)
    assert (one["cls"] == MR.REFINED).sum() > 100
    many = _stage(hip_ctx, 0, neigh[0], p, before=before, band_budget_mb=1)
    _same(many, one, "1 MB bands")
    try:
        refused = _stage(hip_ctx, 0, neigh[0], p, before=before, debug_alloc_limit_mb=2)
    finally:
        hip_ctx.set_option("band_budget_mb", 32768)                 # (forgets the halvings)
    _same(refused, one, "band buffers above 2 MB refused")


# ---------------------------------------------------------------------------------------------- 6. not called, and the cross-check
def test_not_called_nothing_changes_and_the_cross_check_follows(hip_ctx):
    case = cases.get_mvs("mvs_geodesic", **SMALL)
    imgs, ocams, op = cases.oracle_inputs(case)
    neigh = O.mvs_neighbours(ocams, op)
    want = [O.mvs_initial_estimate(imgs, ocams, v, neigh[v], op)[0] for v in range(3)]
    for v in range(3):
        O.mvs_cross_check(imgs, ocams, v, op, want)
    with capi.Context(0) as fresh:                                  # a context that never ran the stage
        cams, p = cases.hip_inputs(case)
        cases.upload_case(fresh, case, cams)
        for v in range(3):
            fresh.mvs_initial_estimate(v, neigh[v], p)
        for v in range(3):
            fresh.mvs_cross_check([0, 1, 2], v, p)
        plain = [fresh.download_depth(v) for v in range(3)]
    for v in range(3):
        ok, msg, _ = cases.compare_depth(plain[v], want[v], 1e-9)
        assert ok, "stage not called, view %d: %s" % (v, msg)
    # with the stage: the cross-check of the refined maps
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    for v in range(3):
        hip_ctx.mvs_initial_estimate(v, neigh[v], p)
    for v in range(3):
        hip_ctx.mvs_view_subpixel(v, neigh[v], p)
    refined = [hip_ctx.download_depth(v) for v in range(3)]
    for v in range(3):
        hip_ctx.mvs_cross_check([0, 1, 2], v, p)
        O.mvs_cross_check(imgs, ocams, v, op, refined)
    moved = 0
    for v in range(3):
        got = hip_ctx.download_depth(v)
        ok, msg, _ = cases.compare_depth(got, refined[v], 1e-9)
        assert ok, "cross-check behind the stage, view %d: %s" % (v, msg)
        moved += int((_bits(got) != _bits(plain[v])).sum())
    assert moved > 100


# ---------------------------------------------------------------------------------------------- 7. the host class
def test_host_class_with_subpixel_equals_the_c_abi_sequence(hip_ctx, tmp_path):
    exe = build_host_program(tmp_path)
    case = cases.get_mvs("mvs_geodesic", w=48, h=36, D=20, nviews=3)
    views = []
    for (rgba, mask, cam, dist, plane) in case["views"]:
        im = rgba.copy()
        im[..., 3] = np.where(mask == 1, 255, 51)                   # the class takes the mask from the alpha channel
        views.append((im, mask, cam, dist, plane))
    case = dict(case, views=views)
    _, ocams, op = cases.oracle_inputs(case)
    neigh = O.mvs_neighbours(ocams, op)
    cams, p = cases.hip_inputs(case)
    inp = str(tmp_path / "in.bin")
    HA._write_input(inp, case, False)
    for mode in ("", "sgm"):
        want = {}
        for on in (1, 0):
            cases.upload_case(hip_ctx, case, cams)
            for v in range(3):
                (hip_ctx.mvs_initial_estimate_peaks if mode else hip_ctx.mvs_initial_estimate)(v, neigh[v], p)
            if mode:
                hip_ctx.mvs_sgm_estimate_views([0, 1, 2])
            infos = [hip_ctx.mvs_view_subpixel(v, neigh[v], p) for v in range(3)] if on else None
            for v in range(3):
                hip_ctx.mvs_cross_check([0, 1, 2], v, p)
            want[on] = ([hip_ctx.download_depth(v) for v in range(3)], infos)
        assert not np.array_equal(_bits(want[1][0][0]), _bits(want[0][0][0]))
        for on in (1, 0):
            outp = str(tmp_path / ("out%d%s.bin" % (on, mode)))
            subprocess.check_call([exe, "compute", inp, outp, str(on)] + ([mode] if mode else []))
            maps, steps = HA._read_output(outp, 3, 48, 36)
            assert steps == list(range(6))
            rec = np.frombuffer(open(outp, "rb").read()[-3 * 64:], np.int64).reshape(3, 8)
            for v in range(3):
                assert np.array_equal(_bits(maps[v]), _bits(want[on][0][v])), (mode, on, v)
                if on:
                    i = want[1][1][v]
                    assert rec[v].tolist() == i["n_class"] + [i["n_moved"], i["n_fallback"]], (mode, v)
                else:
                    assert (rec[v] == 0).all()


# ---------------------------------------------------------------------------------------------- 8. quality
@pytest.mark.parametrize("weight_kind", [1, 0], ids=["geodesic", "adaptive"])
def test_the_quality_scene_on_the_device(hip_ctx, weight_kind):
    """the slanted plane of tests/test_mvs_subpixel_ref.py: in every view median and gated RMS of |z - truth| over the REFINED
    pixels are smaller after the stage, and the figures are the CPU reference's to 1e-7"""
    case, neigh, ref = plane_reference(weight_kind)
    _, ocams, op = cases.oracle_inputs(case)
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    for v in range(3):
        hip_ctx.mvs_initial_estimate(v, neigh[v], p)
        before = hip_ctx.download_depth(v)
        got = _stage(hip_ctx, v, neigh[v], p)
        e = MR.depth_errors(ocams, op, v, neigh[v], before, got, case["gt_depth"][v])
        cpu = ref[v][2]
        print("plane, weights %d, view %d: device %s, CPU reference %s" % (weight_kind, v, e, cpu))
        assert e["median_sub"] < e["median_int"] and e["rms_sub"] < e["rms_int"]
        assert e["n"] == cpu["n"]
        for key in ("median_int", "median_sub", "rms_int", "rms_sub"):
            assert abs(e[key] - cpu[key]) <= 1e-7, key
