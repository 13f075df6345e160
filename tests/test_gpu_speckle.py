"""The speckle filter on the device (srh_view_filter_speckles, options "speckle_min_size" / "speckle_diff_steps" of
srh_twoview_compute) against the NumPy reference (tests/speckle_ref.py): the same bits in the map, the same labels, the
same counters.  The shapes are no multiples of a tile of 16, 32 or 64 and cross its borders on both axes."""
import os

import numpy as np
import pytest

import cases
import filter_ref as F
import speckle_ref as R
from stereoreconstruction_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "bunny_pair.npz")
inf, nan = np.inf, np.nan


class _Params:
    """the depth range of the synthetic maps (made on first use: collecting this file loads nothing)"""
    _p = None

    def __call__(self):
        if _Params._p is None:
            _Params._p = capi.params_twoview(min_depth=30.0, max_depth=80.0, num_depth_levels=100)
        return _Params._p


P = _Params()


def _cam(w, h):
    K = np.array([[w, 0, w / 2], [0, w, h / 2], [0, 0, 1]], np.float64)
    return capi.camera_from_krt(K, np.eye(3), np.zeros(3))


def _upload(ctx, depth, mask=None, slot=0):
    h, w = depth.shape
    rgba = np.zeros((h, w, 4), np.uint8)
    rgba[..., 0] = (np.arange(w) % 251)[None, :]
    rgba[..., 3] = 255
    ctx.upload_view(slot, rgba, mask, _cam(w, h))
    ctx.upload_depth(slot, depth)
    return rgba


def _check(ctx, depth, mask, min_size, max_diff, flags=0, slot=0, labelling=None, tag=""):
    """one call on the map the slot holds (= depth) against the reference -> (filtered map, info)"""
    labels, sizes = labelling if labelling is not None else R.components(depth, mask, max_diff if max_diff > 0 else R.default_max_diff(P()))
    want, winfo = R.apply(depth, labels, sizes, min_size, bool(flags & capi.SPECKLE_TO_NAN))
    info, got_labels = ctx.filter_speckles(slot, P(), min_size, max_diff, flags, want_labels=True)
    got = ctx.download_depth(slot)
    print("%s min_size %d: device %s reference %s" % (tag, min_size, info, winfo))
    assert np.array_equal(got_labels, labels), "%s: %d labels differ" % (tag, (got_labels != labels).sum())
    for k in R.COUNTERS:
        assert info[k] == winfo[k], (tag, k, info, winfo)
    assert R.same_bits(got, want), "%s: %d pixels differ" % (tag, (got.view(np.uint64) != want.view(np.uint64)).sum())
    return got, info


@pytest.mark.parametrize("w,h", [(1, 1), (1, 200), (200, 1), (7, 5)])
def test_degenerate_sizes(hip_ctx, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    d = np.where(rng.random((h, w)) < 0.7, 40.0 + 0.25 * rng.integers(0, 3, (h, w)), inf)
    d[0, 0] = 40.0
    mask = np.ones((h, w), np.uint8)
    if w * h > 1:
        mask.reshape(-1)[1] = 0
    for min_size in (0, 1, 2, 3):
        _upload(hip_ctx, d, mask)
        _check(hip_ctx, d, mask, min_size, 0.25, tag="%dx%d" % (w, h))
    _upload(hip_ctx, d, None)
    _check(hip_ctx, d, None, 2, 0.25, capi.SPECKLE_TO_NAN, tag="%dx%d no mask" % (w, h))


def test_serpentine(hip_ctx):
    d, size = R.serpentine(131, 70)
    _upload(hip_ctx, d)
    got, info = _check(hip_ctx, d, None, size, 0.5, tag="serpentine kept")
    assert R.same_bits(got, d) and info["components"] == 1 and info["largest"] == size == info["valid"]
    got, info = _check(hip_ctx, d, None, size + 1, 0.5, tag="serpentine removed")
    assert not np.isfinite(got).any() and info["removed_pixels"] == size and info["removed_components"] == 1


def test_comb(hip_ctx):
    d = R.comb(131, 70)
    _upload(hip_ctx, d)
    got, info = _check(hip_ctx, d, None, 100, 0.5, tag="comb")
    assert info["components"] == 1 and info["removed_pixels"] == 0 and info["largest"] == 66 * 69 + 131


def test_checkerboard(hip_ctx):
    d = R.checkerboard(67, 35)
    _upload(hip_ctx, d)
    got, info = _check(hip_ctx, d, None, 2, 0.5, tag="checkerboard")
    assert info["removed_components"] == info["valid"] == info["components"] == (67 * 35 + 1) // 2 and info["largest"] == 1
    assert not np.isfinite(got).any()


@pytest.mark.parametrize("w,h", [(130, 66), (640, 480)])
def test_one_plateau(hip_ctx, w, h):
    d = np.full((h, w), 40.0)
    _upload(hip_ctx, d)
    got, info = _check(hip_ctx, d, None, w * h, 0.0, tag="plateau %dx%d" % (w, h))
    assert info == dict(valid=w * h, components=1, removed_components=0, removed_pixels=0, largest=w * h)
    got, info = _check(hip_ctx, d, None, w * h + 1, 0.0, tag="plateau %dx%d removed" % (w, h))
    assert info["removed_pixels"] == w * h and np.isposinf(got).all()


def test_staircase(hip_ctx):
    w, h = 130, 66
    d = R.staircase(w, h)
    _upload(hip_ctx, d)
    got, info = _check(hip_ctx, d, None, h + 1, 0.25, tag="staircase joined")
    assert info["components"] == 1 and info["removed_pixels"] == 0
    got, info = _check(hip_ctx, d, None, h, 0.2, tag="staircase columns kept")
    assert info["components"] == w and info["largest"] == h and info["removed_pixels"] == 0
    got, info = _check(hip_ctx, d, None, h + 1, 0.2, tag="staircase columns removed")
    assert info["removed_components"] == w and info["removed_pixels"] == w * h


def test_corner_straddlers(hip_ctx):
    d = R.corner_straddlers(131, 70)
    _upload(hip_ctx, d)
    got, info = _check(hip_ctx, d, None, 4, 0.5, tag="corners kept")
    assert info["components"] == len(R.CORNERS) == 32 and info["largest"] == 4 and info["removed_pixels"] == 0
    got, info = _check(hip_ctx, d, None, 5, 0.5, capi.SPECKLE_TO_NAN, tag="corners removed")
    assert info["removed_components"] == 32 and info["removed_pixels"] == 128 and np.isnan(got).all()


@pytest.mark.parametrize("w,h", [(333, 257), (1920, 1080)])
def test_random(hip_ctx, w, h):
    mask, d = R.random_map(w, h, 0x5EC0 + w)
    valid = R.valid_pixels(d, mask)
    assert 0.25 < 1 - valid.mean() < 0.4
    assert np.isposinf(d).any() and np.isnan(d).any() and (d == -1).any() and (mask == 0).any()
    labelling = R.components(d, mask, R.RANDOM_MAX_DIFF)
    _, info5 = R.apply(d, *labelling, 5)
    assert info5["components"] > 100 and 0 < info5["removed_components"] < info5["components"]
    _upload(hip_ctx, d, mask)
    for min_size in (2, 5, 50, 10**9):
        for flags in (0, capi.SPECKLE_TO_NAN):
            hip_ctx.upload_depth(0, d)
            got, info = _check(hip_ctx, d, mask, min_size, R.RANDOM_MAX_DIFF, flags, labelling=labelling,
                               tag="random %dx%d flags %d" % (w, h, flags))
            # what is not valid is never written
            assert R.same_bits(got[~valid], d[~valid])
    assert info["removed_pixels"] == info["valid"]                  # min_size 10**9


def test_default_max_diff_is_two_depth_steps(hip_ctx):
    mask, d = R.random_map(150, 90, 77)
    _upload(hip_ctx, d, mask)
    two = R.default_max_diff(P())
    a, ia = _check(hip_ctx, d, mask, 5, 0.0, tag="default max_diff")
    hip_ctx.upload_depth(0, d)
    b, ib = _check(hip_ctx, d, mask, 5, two, tag="explicit two steps")
    assert R.same_bits(a, b) and ia == ib


def test_idempotence_and_purity(hip_ctx):
    case = cases.get_twoview("geodesic_masks", w=72, h=40, D=16)
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    hip_ctx.set_option("wta_outputs", capi.WTA_WINNERS | capi.WTA_COSTS)
    try:
        hip_ctx.twoview_compute(0, 1, p)
    finally:
        hip_ctx.set_option("wta_outputs", 0)
    before = hip_ctx.wta_outputs(0)
    image, mask = hip_ctx.download_view_image(0)
    mask2, d = R.random_map(72, 40, 5)
    d[mask == 0] = 45.0                                  # fine depths under the slot's own mask: they must stay
    hip_ctx.upload_depth(0, d)
    info = hip_ctx.filter_speckles(0, P(), 5, R.RANDOM_MAX_DIFF)
    once = hip_ctx.download_depth(0)
    want, _, winfo = R.filter_map(d, mask, 5, R.RANDOM_MAX_DIFF)
    assert R.same_bits(once, want) and info == winfo and 0 < info["removed_pixels"] < info["valid"]
    again = hip_ctx.filter_speckles(0, P(), 5, R.RANDOM_MAX_DIFF)
    assert again["removed_pixels"] == 0 and again["removed_components"] == 0
    assert again["valid"] == info["valid"] - info["removed_pixels"]
    assert R.same_bits(hip_ctx.download_depth(0), once)
    hip_ctx.upload_depth(0, d)
    assert hip_ctx.filter_speckles(0, P(), 5, R.RANDOM_MAX_DIFF) == info and R.same_bits(hip_ctx.download_depth(0), once)
    after = hip_ctx.wta_outputs(0)
    assert sorted(after) == sorted(before) and len(before) == 4
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    image2, mask_after = hip_ctx.download_view_image(0)
    assert np.array_equal(image, image2) and np.array_equal(mask, mask_after)


def test_bad_arguments(hip_ctx):
    d = np.full((8, 8), 40.0)
    _upload(hip_ctx, d)
    for kw in (dict(min_size=-1), dict(min_size=2, flags=2), dict(min_size=2, max_diff=inf), dict(min_size=2, max_diff=nan)):
        with pytest.raises(capi.StereoHipError) as e:
            hip_ctx.filter_speckles(0, P(), **kw)
        assert e.value.code == capi.SRH_E_INVALID
    with pytest.raises(capi.StereoHipError) as e:
        hip_ctx.filter_speckles(capi.MAX_VIEWS - 1, P(), 2)               # an empty slot
    assert e.value.code == capi.SRH_E_INVALID
    one = capi.params_twoview(min_depth=30.0, max_depth=80.0, num_depth_levels=1)
    with pytest.raises(capi.StereoHipError) as e:
        hip_ctx.filter_speckles(0, one, 2)                              # the default max_diff needs two levels ...
    assert e.value.code == capi.SRH_E_INVALID
    assert hip_ctx.filter_speckles(0, one, 2, 0.5)["components"] == 1   # ... an explicit one does not
    for name, value in (("speckle_min_size", -1), ("speckle_diff_steps", 0)):
        with pytest.raises(capi.StereoHipError):
            hip_ctx.set_option(name, value)
    assert R.same_bits(hip_ctx.download_depth(0), d)


def _load_bunny():
    g = np.load(GOLD)
    views = []
    for tag in ("left", "right"):
        views.append((g[tag + "_rgba"], g[tag + "_mask"], (g[tag + "_K"], g[tag + "_R"], g[tag + "_t"]),
                      g[tag + "_dist"], None))
    params = dict(min_depth=30.0, max_depth=80.0, num_depth_levels=100, image_scale=float(g["scale"][0]),
                  window_radius=5, weight_kind=1)
    return dict(name="bunny", kind="twoview", views=views, params=params)


def test_pipeline_option_on_the_bunny_pair(hip_ctx):
    case = _load_bunny()
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    masks = [case["views"][s][1] for s in (0, 1)]
    plain = hip_ctx.twoview_compute(0, 1, p)
    want = [R.filter_map(plain[s], masks[s], 20, R.default_max_diff(p, 2)) for s in (0, 1)]
    assert all(0 < w[2]["removed_pixels"] < w[2]["valid"] for w in want)
    steps = []
    hip_ctx.set_hooks(progress=lambda s, stage: steps.append((s, stage if isinstance(stage, str) else stage.decode())))
    try:
        hip_ctx.set_option("speckle_min_size", 20)
        got = hip_ctx.twoview_compute(0, 1, p)
        assert [s for s, _ in steps] == [1, 3, 5, 5, 8] and steps[3][1] == "Removing speckles..."
        for s in (0, 1):
            assert R.same_bits(got[s], want[s][0]), "slot %d" % s
            assert R.same_bits(hip_ctx.download_depth(s), want[s][0])
        # three steps: another max_diff, another result
        hip_ctx.set_option("speckle_diff_steps", 3)
        got3 = hip_ctx.twoview_compute(0, 1, p)
        for s in (0, 1):
            assert R.same_bits(got3[s], R.filter_map(plain[s], masks[s], 20, R.default_max_diff(p, 3))[0])
        hip_ctx.set_option("speckle_diff_steps", 2)
        # with the hole filling behind it
        hip_ctx.set_option("filter_invalid", 3)
        del steps[:]
        filled = hip_ctx.twoview_compute(0, 1, p)
        assert [s for s, _ in steps] == [1, 3, 5, 5, 6, 7, 8]
        for s in (0, 1):
            assert R.same_bits(filled[s], F.filter_map(case["views"][s][0], masks[s], want[s][0], F.oparams(p), 3)), "slot %d" % s
    finally:
        hip_ctx.set_option("speckle_min_size", 0)
        hip_ctx.set_option("speckle_diff_steps", 2)
        hip_ctx.set_option("filter_invalid", 0)
        hip_ctx.set_hooks()
    del steps[:]
    again = hip_ctx.twoview_compute(0, 1, p)
    assert R.same_bits(again[0], plain[0]) and R.same_bits(again[1], plain[1])


def test_pipeline_option_on_the_label_volume_stages(hip_ctx):
    case = cases.get_twoview("geodesic_masks", w=72, h=40, D=16)
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    masks = [case["views"][s][1] for s in (0, 1)]
    for run in (hip_ctx.twoview_compute_sgm, hip_ctx.twoview_compute_mrf):
        plain = run(0, 1, p)[:2]
        # these maps are smooth: the smallest min_size that removes something (the smallest component of the two maps)
        sizes = np.concatenate([R.components(plain[s], masks[s], R.default_max_diff(p, 2))[1] for s in (0, 1)])
        min_size = int(sizes[sizes > 0].min()) + 1
        hip_ctx.set_option("speckle_min_size", min_size)
        try:
            got = run(0, 1, p)[:2]
        finally:
            hip_ctx.set_option("speckle_min_size", 0)
        removed = 0
        for s in (0, 1):
            want, _, info = R.filter_map(plain[s], masks[s], min_size, R.default_max_diff(p, 2))
            removed += info["removed_pixels"]
            assert R.same_bits(got[s], want), "slot %d" % s
        print("%s: min_size %d removes %d pixels" % (run.__name__, min_size, removed))
        assert removed > 0


def test_multiview_maps_after_the_cross_check(hip_ctx):
    case = cases.get_mvs("mvs_geodesic", w=40, h=28, D=12, nviews=3)
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    neigh = capi.mvs_neighbours(cams, p)
    nv = len(cams)
    for v in range(nv):
        hip_ctx.mvs_initial_estimate(v, neigh[v], p)
    for v in range(nv):
        hip_ctx.mvs_cross_check(list(range(nv)), v, p)
    removed = 0
    for v in range(nv):
        d = hip_ctx.download_depth(v).copy()
        mask = case["views"][v][1]
        fin = np.argwhere(np.isfinite(d) & (d > 0) & (mask == 1))
        assert len(fin) > 50
        for y, x in fin[::17]:                             # "no peak" pixels, also where the run left none
            d[y, x] = -1.0
        hip_ctx.upload_depth(v, d)
        info = hip_ctx.filter_speckles(v, p, 8, 0.0, capi.SPECKLE_TO_NAN)
        got = hip_ctx.download_depth(v)
        want, _, winfo = R.filter_map(d, mask, 8, R.default_max_diff(p), to_nan=True)
        assert R.same_bits(got, want) and info == winfo
        assert (got[d == -1] == -1).all() and not np.isposinf(got[np.isfinite(d)]).any()
        assert np.isnan(got[np.isfinite(d) & (d > 0) & (mask == 1)]).sum() == info["removed_pixels"]
        removed += info["removed_pixels"]
    assert removed > 0
