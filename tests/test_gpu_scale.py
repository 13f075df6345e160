"""Views scaled on the device in Qt's arithmetic (srh_scale.hip): the kernels against Qt's own outputs
(tests/golden/qt_scale.npz, made by tests/golden/make_qt_scale.py) and against the numpy restatement
(tests/qt_scale_ref.py, which tests/test_qt_scale_restatement.py holds to the installed Qt) -- byte for byte.
Reads neither Qt nor the reference tree."""
import os
import zlib

import numpy as np
import pytest

import qt_scale_ref as R
from stereoreconstruction_amd import capi
from stereoreconstruction_amd import synthetic as S

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qt_scale.npz")
SYNTHETIC = {"rand64": (64, 48, 101), "rand101": (101, 77, 102), "rand37": (37, 29, 103)}      # w, h, seed (make_qt_scale.py)


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    src = {k: R.synthetic_source(*v) for k, v in SYNTHETIC.items()}
    src["bunny"] = g["bunny_src"]
    for k, v in src.items():
        assert zlib.crc32(v.tobytes()) == int(g[k + "_crc"][0]), "source %s is not the one the fixture was made from" % k
    return g, src


def same(got, want, what):
    assert got.shape == want.shape, "%s: shape %s, want %s" % (what, got.shape, want.shape)
    bad = int((got != want).any(axis=-1).sum()) if got.ndim == 3 else int((got != want).sum())
    assert bad == 0, "%s: %d pixels differ" % (what, bad)


def camera():
    (K, Rm, t), _ = S.rectified_cameras(64, 48)
    return capi.camera_from_krt(K, Rm, t, None)


@pytest.mark.parametrize("name", ["rand64", "rand101", "rand37", "bunny"])
def test_fixture_cases(hip_ctx, gold, name):
    g, src = gold
    scale = float(g[name + "_scale"][0])
    for mode, mtag in ((capi.SCALE_SMOOTH, "smooth"), (capi.SCALE_FAST, "fast")):
        for alpha, atag in ((1, "alpha"), (0, "opaque")):
            want = g["%s_%s_%s" % (name, mtag, atag)]
            same(R.scale_image(src[name], alpha, scale, mode), want, "restatement %s %s %s" % (name, mtag, atag))
            same(hip_ctx.scale_image(src[name], alpha, scale, mode), want, "device %s %s %s" % (name, mtag, atag))


def test_premultiply_every_channel_alpha_pair(hip_ctx):
    """Every (channel, alpha) pair through the device's premultiplication: at scale 0.5 an even image whose 2x2 blocks are
    constant scales to the premultiplied blocks themselves (two taps of weight 8192 per axis: c*8192*2 >> 4, times 8192*2,
    >> 24 is c), so the smooth scale of the blown-up table is the restatement's premultiplied table."""
    c, a = np.meshgrid(np.arange(256), np.arange(256))
    table = np.stack([c, 255 - c, (c*7) % 256, a], axis=-1).astype(np.uint8)
    big = np.ascontiguousarray(table.repeat(2, axis=0).repeat(2, axis=1))
    same(hip_ctx.scale_image(big, 1, 0.5, capi.SCALE_SMOOTH), R.premultiply(table), "premultiplied table")
    same(R.scale_image(big, 1, 0.5, R.SMOOTH), R.premultiply(table), "premultiplied table, restatement")


# 333x251 at 0.41: a ragged tile edge in both axes; 1175x881 at 0.3: a shape whose fast-scaled rows an integer step misplaces;
# 17x9 at 0.6: a target smaller than a tile; 300x200 at 0.2: a target exactly one tile wide (60 columns of the 64);
# 2600x45 at 0.025: a tile whose source rows and columns go by in several chunks and staged pieces; 4200x6 at 0.5: a target
# of 2100 columns, so that the fast scale with alpha re-places its columns once, at target column 2048
@pytest.mark.parametrize("w,h,scale", [(333, 251, 0.41), (1175, 881, 0.3), (17, 9, 0.6), (300, 200, 0.2), (2600, 45, 0.025),
                                       (4200, 6, 0.5)])
def test_shapes_against_restatement(hip_ctx, w, h, scale):
    rng = np.random.default_rng(w*1000 + h)
    src = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    src[..., 3][rng.random((h, w)) < 0.75] = 255
    for mode in (capi.SCALE_SMOOTH, capi.SCALE_FAST):
        assert capi.scaled_size(w, h, scale, mode) == R.scaled_size(w, h, scale, mode)
        for alpha in (1, 0):
            same(hip_ctx.scale_image(src, alpha, scale, mode), R.scale_image(src, alpha, scale, mode),
                 "%dx%d at %g mode %d alpha %d" % (w, h, scale, mode, alpha))


def test_upload_scaled_mask_rules(hip_ctx, gold):
    g, src = gold
    cam = camera()
    # MultiViewStereo's rule; 101x77 at 0.5: the image is 50x39, the fast copy 50x38 -- the last row is not WHITE
    for name in ("rand101", "bunny", "rand64"):
        scale = float(g[name + "_scale"][0])
        for alpha in (1, 0):
            hip_ctx.upload_view_scaled(4, src[name], alpha, scale, cam, capi.MASK_ALPHA_FAST)
            img, mask = R.ingest(src[name], alpha, scale, R.MASK_ALPHA_FAST)
            assert hip_ctx.view_size(4) == (img.shape[1], img.shape[0])
            got_img, got_mask = hip_ctx.download_view_image(4)
            same(got_img, img, name + " image")
            same(got_mask, mask, name + " alpha mask")
            same(got_img, g["%s_smooth_%s" % (name, "alpha" if alpha else "opaque")], name + " image against Qt")
            if alpha:
                fast = g[name + "_fast_alpha"]
                want = np.zeros(mask.shape, np.uint8)
                want[:fast.shape[0]] = fast[..., 3] == 255
                same(got_mask, want, name + " alpha mask against Qt")
    img, mask = R.ingest(src["rand101"], 1, 0.5, R.MASK_ALPHA_FAST)
    assert img.shape[:2] == (39, 50) and not mask[38].any() and mask[:38].any()
    # TwoViewStereo's rule: a mask image of its own, smooth-scaled; here of the image's size, smaller, and absent
    rng = np.random.default_rng(5)
    for mw, mh in ((101, 77), (90, 60)):
        m = np.full((mh, mw, 4), 255, np.uint8)
        m[rng.random((mh, mw)) < 0.3] = (0, 0, 0, 255)
        m[mh//2:, :mw//3] = (255, 255, 255, 255)                            # a solid WHITE block survives the averaging
        hip_ctx.upload_view_scaled(4, src["rand101"], 1, 0.5, cam, capi.MASK_IMAGE_SMOOTH, m, False)
        img, mask = R.ingest(src["rand101"], 1, 0.5, R.MASK_IMAGE_SMOOTH, m, False)
        assert 0 < mask.sum() < mask.size
        got_img, got_mask = hip_ctx.download_view_image(4)
        same(got_img, img, "image under the mask-image rule")
        same(got_mask, mask, "mask image %dx%d" % (mw, mh))
    for rule, m in ((capi.MASK_IMAGE_SMOOTH, None), (capi.MASK_NONE, None)):
        hip_ctx.upload_view_scaled(4, src["rand101"], 1, 0.5, cam, rule, m)
        got_img, got_mask = hip_ctx.download_view_image(4)
        same(got_img, g["rand101_smooth_alpha"], "image, no mask")
        assert (got_mask == 1).all()


def test_pair_depth_maps_same_bits(hip_ctx, gold):
    """The fixture crop and a shifted copy through upload_view_scaled give the depth maps that the same pair, scaled by
    the restatement and sent through srh_view_upload, gives -- bit for bit."""
    g, src = gold
    left = src["bunny"]
    right = np.roll(left, -24, axis=1)                                      # 6 pixels at scale 0.25
    scale, D = 0.25, 16
    (Kl, Rl, tl), (Kr, Rr, tr) = S.rectified_cameras(64, 48)
    Kl = Kl.copy(); Kr = Kr.copy()
    Kl[:2] /= scale; Kr[:2] /= scale                                        # the cameras describe the file-resolution image
    cams = [capi.camera_from_krt(Kl, Rl, tl, None), capi.camera_from_krt(Kr, Rr, tr, None)]
    zmin, zmax = S.rectified_depth_range(64, D)
    p = capi.params_twoview(min_depth=zmin, max_depth=zmax, num_depth_levels=D, image_scale=scale)
    for slot, im in enumerate((left, right)):
        img, mask = R.ingest(im, 1, scale, R.MASK_ALPHA_FAST)
        assert 0 < mask.sum() < mask.size
        hip_ctx.upload_view(slot, img, mask, cams[slot])
    want = hip_ctx.twoview_compute(0, 1, p)
    for slot, im in enumerate((left, right)):
        hip_ctx.upload_view_scaled(2 + slot, im, 1, scale, cams[slot], capi.MASK_ALPHA_FAST)
    got = hip_ctx.twoview_compute(2, 3, p)
    assert np.isfinite(want[0]).sum() > 50
    for a, b, tag in ((got[0], want[0], "left"), (got[1], want[1], "right")):
        assert a.shape == b.shape == (48, 64)
        assert (a.view(np.uint64) == b.view(np.uint64)).all(), tag


def test_identity_passes_bytes_through(hip_ctx, gold):
    _, src = gold
    im = src["rand64"]
    for scale in (1.0, 1.01):
        for mode in (capi.SCALE_SMOOTH, capi.SCALE_FAST):
            same(hip_ctx.scale_image(im, 1, scale, mode), im, "identity with alpha")
            opaque = im.copy()
            opaque[..., 3] = 255
            same(hip_ctx.scale_image(im, 0, scale, mode), opaque, "identity, opaque")
    hip_ctx.upload_view_scaled(4, im, 1, 1.0, camera(), capi.MASK_ALPHA_FAST)
    got_img, got_mask = hip_ctx.download_view_image(4)
    same(got_img, im, "identity upload")
    same(got_mask, (im[..., 3] == 255).astype(np.uint8), "identity upload, alpha mask")


def test_refused_shapes_leave_the_slot(hip_ctx, gold):
    _, src = gold
    cam = camera()
    im = src["rand64"]
    hip_ctx.upload_view_scaled(5, im, 1, 0.25, cam, capi.MASK_ALPHA_FAST)
    before = hip_ctx.download_view_image(5)
    thin = np.ascontiguousarray(im[:1])                                     # 64x1: no strict downscale in y
    for args, code in (((im, 1, 1.5), capi.SRH_E_UNSUPPORTED), ((im, 1, 0.0), capi.SRH_E_INVALID), ((im, 1, 0.01), capi.SRH_E_INVALID),
                       ((im, 1, -1.0), capi.SRH_E_INVALID), ((thin, 1, 0.7), capi.SRH_E_UNSUPPORTED)):
        with pytest.raises(capi.StereoHipError) as e:
            hip_ctx.upload_view_scaled(5, args[0], args[1], args[2], cam, capi.MASK_ALPHA_FAST)
        assert e.value.code == code, args[2]
        with pytest.raises(capi.StereoHipError) as e:
            hip_ctx.scale_image(*args)
        assert e.value.code == code, args[2]
    # a mask image that cannot be scaled refuses the whole upload; so does an unknown rule
    with pytest.raises(capi.StereoHipError) as e:
        hip_ctx.upload_view_scaled(5, im, 1, 0.7, cam, capi.MASK_IMAGE_SMOOTH, thin, False)
    assert e.value.code == capi.SRH_E_UNSUPPORTED
    with pytest.raises(capi.StereoHipError) as e:
        hip_ctx.upload_view_scaled(5, im, 1, 0.25, cam, 7)
    assert e.value.code == capi.SRH_E_INVALID
    assert hip_ctx.view_size(5) == (16, 12)
    after = hip_ctx.download_view_image(5)
    same(after[0], before[0], "slot image after the refusals")
    same(after[1], before[1], "slot mask after the refusals")
