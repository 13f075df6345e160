"""tests/qt_scale_ref.py against the installed Qt, byte for byte.

The driver tests/qt_scale_driver.cpp is compiled here against the Qt that oracle/Makefile names; without that Qt the
module skips.  Both modes of QImage::scaledToWidth, sizes included, and convertToFormat(Format_ARGB32_Premultiplied).

The sweep: widths 16 ... 1300 with heights 3w/4 + {0, 1, 2} at seven scales, with and without alpha.  The fast scale is
cheap and takes every 29th width; the smooth scale takes every 97th plus every width of the six shapes on which the
integer row rule of the fast scale is known to fail (the arithmetic of an axis depends on its two lengths only, and the
sweep's heights give the vertical axis a second, unrelated set of length pairs)."""
import os

import numpy as np
import pytest

import qt_scale_qt
import qt_scale_ref as R

pytestmark = pytest.mark.skipif(not qt_scale_qt.available(), reason="needs the Qt that oracle/Makefile names")

SCALES = [0.125, 0.25, 1.0/3.0, 0.3, 0.41, 0.5, 0.77]
TEN_CASES = [(64, 48, 0.25), (64, 48, 0.5), (101, 77, 0.5), (101, 77, 0.3), (1024, 768, 0.25), (1024, 768, 0.7),
             (37, 29, 0.7), (37, 29, 0.25), (200, 120, 0.3), (200, 120, 0.5)]
# source shapes and target widths on which stepping the fast scale's rows in 16.16 fixed point goes wrong
RESIDUAL = [(787, 591, 605), (981, 736, 755), (1078, 809, 830), (1175, 881, 352), (1175, 882, 904), (1272, 955, 979)]
REF_BUNNY = "/root/reference/example/images/bunny"


@pytest.fixture(scope="module")
def qt(tmp_path_factory):
    return qt_scale_qt.Qt(tmp_path_factory.mktemp("qt_scale"))


def check(qt, img, alpha, scale, mode, dw=None):
    h, w = img.shape[:2]
    if dw is None:
        dw = int(w*scale)
    else:
        scale = (dw + 0.5)/w
        assert int(w*scale) == dw
    want = qt.scaled_to_width(img, alpha, dw, mode == R.SMOOTH)
    got = R.scale_image(img, alpha, scale, mode)
    assert R.scaled_size(w, h, scale, mode) == (want.shape[1], want.shape[0]), (w, h, scale, mode)
    assert got.shape == want.shape
    bad = int((got != want).any(axis=-1).sum())
    assert bad == 0, "%dx%d scale %g mode %d alpha %d: %d pixels differ" % (w, h, scale, mode, alpha, bad)


def test_qt_version(qt):
    # DESIGN.md 4f names the version the arithmetic was pinned to; another Qt may still agree, and then this line moves
    assert qt.version.startswith("5.9."), qt.version


def test_premultiply(qt):
    c, a = np.meshgrid(np.arange(256), np.arange(256))
    img = np.stack([c, 255 - c, (c*7) % 256, a], axis=-1).astype(np.uint8)      # every (channel, alpha) pair
    assert (qt.premultiply(img) == R.premultiply(img)).all()


@pytest.mark.parametrize("alpha", [0, 1])
@pytest.mark.parametrize("mode", [R.SMOOTH, R.FAST])
def test_ten_cases_and_residual_shapes(qt, mode, alpha):
    rng = np.random.default_rng(7)
    for w, h, s in TEN_CASES:
        check(qt, qt_scale_qt.random_image(rng, w, h, alpha), alpha, s, mode)
    for w, h, dw in RESIDUAL:
        check(qt, qt_scale_qt.random_image(rng, w, h, alpha), alpha, None, mode, dw=dw)


def test_residual_rows_named_by_coordinates(qt):
    """Every source pixel carries its own coordinates: the fast-scaled image then names the source row of every target
    row, and the restatement's row map must be that list -- on the six shapes where the integer rule is not."""
    wrong = 0
    for w, h, dw in RESIDUAL:
        y, x = np.mgrid[0:h, 0:w]
        img = np.stack([x & 255, (x >> 8) | ((y >> 8) << 4), y & 255, np.full_like(x, 255)], axis=-1).astype(np.uint8)
        q = qt.scaled_to_width(img, 1, dw, False).astype(np.int64)
        rows = (q[..., 2] | ((q[..., 1] >> 4) << 8))[:, 0]
        cols = (q[..., 0] | ((q[..., 1] & 15) << 8))[0]
        xs, ys = R.fast_maps(w, h, dw, q.shape[0], True)
        assert (ys == rows).all() and (xs == cols).all(), (w, h, dw)
        m = int((1.0/(dw/float(w)))*65536.0)
        wrong += int((((m*np.arange(q.shape[0]) + m//2 - 1) >> 16) != rows).sum())
    assert wrong == 12                                       # the residual the integer rule leaves (4 + 1 + 3 + 1 + 2 + 1 rows)


@pytest.mark.parametrize("scale", SCALES)
def test_sweep_fast(qt, scale):
    rng = np.random.default_rng(11)
    for w in range(16, 1301, 29):
        for k in (0, 1, 2):
            h = 3*w//4 + k
            for alpha in (0, 1):
                if int(w*scale) < 1:
                    continue
                check(qt, qt_scale_qt.random_image(rng, w, h, alpha), alpha, scale, R.FAST)


@pytest.mark.parametrize("scale", SCALES)
def test_sweep_smooth(qt, scale):
    rng = np.random.default_rng(13)
    widths = sorted(set(range(16, 1301, 97)) | {w for w, _, _ in RESIDUAL} | {1300})
    for w in widths:
        for k in (0, 1, 2):
            h = 3*w//4 + k
            for alpha in (0, 1):
                check(qt, qt_scale_qt.random_image(rng, w, h, alpha), alpha, scale, R.SMOOTH)


def test_wide_target_spans(qt):
    # a target row wider than 2048 pixels is drawn in pieces, each placed anew (fast scale, with alpha)
    rng = np.random.default_rng(17)
    for w, dw in ((4090, 3777), (4000, 3001)):
        check(qt, qt_scale_qt.random_image(rng, w, 12, 1), 1, None, R.FAST, dw=dw)


@pytest.mark.parametrize("alpha", [0, 1])
def test_identity(qt, alpha):
    rng = np.random.default_rng(19)
    img = qt_scale_qt.random_image(rng, 40, 30, alpha)
    for scale in (1.0, 1.02):                                # (int)(40*1.02) == 40
        for mode in (R.SMOOTH, R.FAST):
            want = qt.scaled_to_width(img, alpha, int(40*scale), mode == R.SMOOTH)
            assert (R.scale_image(img, alpha, scale, mode) == want).all()
            assert R.scaled_size(40, 30, scale, mode) == (40, 30)


def test_refused_shapes():
    for args, code in [((64, 48, 0.0), R.E_INVALID), ((64, 48, 0.01), R.E_INVALID), ((64, 48, -0.5), R.E_INVALID),
                       ((64, 48, 1.5), R.E_UNSUPPORTED), ((64, 1, 0.7), R.E_UNSUPPORTED), ((0, 4, 0.5), R.E_INVALID)]:
        for mode in (R.SMOOTH, R.FAST):
            with pytest.raises(R.Refused) as e:
                R.scaled_size(*args, mode=mode)
            assert e.value.code == code, (args, mode)
    # a height the fast mode rounds to nothing
    with pytest.raises(R.Refused) as e:
        R.scaled_size(64, 3, 0.125, R.FAST)
    assert e.value.code == R.E_INVALID
    assert R.scaled_size(64, 3, 0.125, R.SMOOTH) == (8, 1)


@pytest.mark.skipif(not os.path.isdir(REF_BUNNY), reason="example images live in the reference tree")
def test_bunny_ingest():
    """The whole MultiViewStereo ingest of two example images equals the committed fixture (made by the Qt binding)."""
    from PIL import Image
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bunny_pair.npz"))
    for side, cam in (("left", "7310085"), ("right", "7310087")):
        im = Image.open(os.path.join(REF_BUNNY, cam + ".png"))
        alpha = "A" in im.getbands()
        src = np.asarray(im.convert("RGBA"))
        img, mask = R.ingest(src, alpha, float(g["scale"][0]), R.MASK_ALPHA_FAST)
        assert img.shape == g[side + "_rgba"].shape
        assert (img == g[side + "_rgba"]).all(), side
        assert (mask == g[side + "_mask"]).all(), side
