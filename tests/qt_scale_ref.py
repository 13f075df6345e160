"""numpy restatement of the image scaling at the top of the reference's path: what Qt 5.9.7's
QImage::scaledToWidth does in its two modes to a 32-bit image, the integer premultiplication that precedes the smooth
scale of an image with alpha, and the reference's three mask rules.  Own code, written from the arithmetic as DESIGN.md
states it; tests/test_qt_scale_restatement.py holds it to the installed Qt byte for byte, tests/test_gpu_scale.py holds
the device kernels to it.

Pixels are (h, w, 4) uint8 arrays of R, G, B, A bytes -- the layout of srh_view_upload.  Every run sum asserts that its
last tap lies inside the image."""
import math

import numpy as np

SMOOTH, FAST = 0, 1                      # SRH_SCALE_SMOOTH, SRH_SCALE_FAST
MASK_NONE, MASK_ALPHA_FAST, MASK_IMAGE_SMOOTH = 0, 1, 2   # SRH_MASK_*
E_INVALID, E_UNSUPPORTED = -1, -5        # SRH_E_*


class Refused(Exception):
    """The shape is outside what the library scales; .code is the SRH_E_* value the C-ABI returns for it."""

    def __init__(self, code, msg):
        Exception.__init__(self, msg)
        self.code = code


def scaled_size(sw, sh, image_scale, mode=SMOOTH):
    """(w, h) of scaledToWidth((int)(sw*image_scale), mode) of an sw x sh image.  w == sw: the identity."""
    if sw <= 0 or sh <= 0:
        raise Refused(E_INVALID, "empty source")
    t = float(sw)*float(image_scale)
    if not math.isfinite(t) or abs(t) >= 2**31:
        raise Refused(E_INVALID, "scale out of range")
    dw = int(t)                                            # C++ truncation toward zero
    if dw <= 0:
        raise Refused(E_INVALID, "target width %d" % dw)
    if dw == sw:
        return sw, sh
    if dw > sw:
        raise Refused(E_UNSUPPORTED, "up-scaling")
    f = float(dw)/float(sw)
    dh = int(f*sh + 0.9999) if mode == SMOOTH else int(math.floor(f*sh + 0.5))
    if dh >= sh or dh <= 0:
        raise Refused(E_UNSUPPORTED if dh > 0 else E_INVALID, "target height %d of %d" % (dh, sh))
    return dw, dh


def premultiply(rgba):
    """Qt's integer ARGB32 -> ARGB32_Premultiplied, per channel pair; alpha kept."""
    px = rgba.astype(np.uint32)
    a = px[..., 3]
    # the two channel pairs of a QRgb word are (R, B) and (A -> replaced, G); per channel the rule is the same
    out = np.empty_like(rgba)
    for c in range(3):
        t = px[..., c]*a
        out[..., c] = ((t + ((t >> 8) & 0xff) + 0x80) >> 8).astype(np.uint8)
    out[..., 3] = rgba[..., 3]
    return out


def axis_taps(s, d):
    """Per target index of an axis scaled down from s to d: first tap p, and the weights of its run (row i: w[i, :n[i]])."""
    assert 0 < d < s
    inc = (s << 16)//d
    cp = ((d << 14) + s - 1)//s
    i = np.arange(d, dtype=np.int64)
    val = i*inc
    p = val >> 16
    ap = ((0x10000 - (val & 0xffff))*cp) >> 16
    j = (1 << 14) - ap
    assert (j > 0).all()
    mid = (j - 1)//cp                                      # taps of weight Cp: while (j > Cp)
    last = j - mid*cp                                      # the last tap's weight, in (0, Cp]
    n = mid + 2
    L = int(n.max())
    w = np.zeros((d, L), dtype=np.int64)
    w[:, 0] = ap
    k = np.arange(1, L, dtype=np.int64)[None, :]
    w[:, 1:] = np.where(k <= mid[:, None], cp, 0)
    w[i, mid + 1] = last
    assert (w.sum(axis=1) == 1 << 14).all()
    assert (p + n - 1 < s).all(), "a run's last tap leaves the image (s = %d, d = %d)" % (s, d)
    return p, n, w


def smooth_scale(rgba, dw, dh):
    """The smooth (area-averaging) downscale of raw 32-bit pixels to dw x dh, strict in both axes."""
    sh, sw = rgba.shape[:2]
    px, nx, wx = axis_taps(sw, dw)
    py, ny, wy = axis_taps(sh, dh)
    src = rgba.astype(np.uint32)
    wx, wy = wx.astype(np.uint32), wy.astype(np.uint32)
    hor = np.zeros((sh, dw, 4), dtype=np.uint32)               # a run sum is at most 255 << 14
    for k in range(wx.shape[1]):
        col = np.minimum(px + k, sw - 1)                   # (weight 0 beyond the run: the clamp is never a tap)
        hor += src[:, col, :]*wx[None, :, k, None]
    hor >>= 4
    out = np.zeros((dh, dw, 4), dtype=np.uint32)               # the vertical total is an unsigned 32-bit word: it wraps as one
    for k in range(wy.shape[1]):
        row = np.minimum(py + k, sh - 1)
        out += hor[row, :, :]*wy[:, k, None, None]
    return (out >> 24).astype(np.uint8)


def fast_maps(sw, sh, dw, dh, has_alpha):
    """Source column of every target column and source row of every target row of the fast (nearest-neighbour) scale.

    Qt 5.9 draws the source through a QPainter with the scale set.  An image WITH alpha (Format_ARGB32) takes the raster
    engine's span path: the inverse of translate(1/65536) * scale(f) is applied in doubles at the centre of the first
    pixel of every span piece (a row, cut into pieces of 2048 pixels), then stepped along x in 16.16 fixed point -- so
    rows are placed in doubles, one by one, and columns by an integer step.  An image WITHOUT alpha (Format_RGB32) takes
    the integer blitter, which steps both axes in 16.16 fixed point."""
    f = float(dw)/float(sw)
    if has_alpha:
        inv = 1.0/f
        off = -((1.0/65536.0)*f)*inv
        step = int(inv*65536.0)
        xs = np.empty(dw, dtype=np.int64)
        fx = 0
        for i in range(dw):
            if i % 2048 == 0:
                fx = int((inv*(i + 0.5) + off)*65536.0)
            xs[i] = fx >> 16
            fx += step
        ys = np.array([int((inv*(j + 0.5) + off)*65536.0) >> 16 for j in range(dh)], dtype=np.int64)
    else:
        maps = []
        for s, d in ((sw, dw), (sh, dh)):
            scale = (f*s)/s                                # target extent / source extent, as the blitter forms it
            m = int(65536.0/scale)
            first = int(math.ceil(0.5*m)) - 1
            maps.append((first + m*np.arange(d, dtype=np.int64)) >> 16)
        xs, ys = maps
    assert xs.min() >= 0 and xs.max() < sw and ys.min() >= 0 and ys.max() < sh, "a fast-scale tap leaves the image"
    return xs, ys


def fast_scale(rgba, dw, dh, has_alpha):
    """The fast scale to dw x dh.  With alpha, a fully transparent pixel comes out as four zero bytes (the painter skips it
    over the zero-filled target); every other pixel is the source's bytes."""
    sh, sw = rgba.shape[:2]
    xs, ys = fast_maps(sw, sh, dw, dh, has_alpha)
    out = rgba[ys][:, xs].copy()
    if has_alpha:
        out[out[..., 3] == 0] = 0
    else:
        out[..., 3] = 255
    return out


def scale_image(rgba, has_alpha, image_scale, mode=SMOOTH):
    """QImage(rgba).scaledToWidth((int)(w*image_scale), mode) as raw R, G, B, A bytes.  Raises Refused."""
    sh, sw = rgba.shape[:2]
    dw, dh = scaled_size(sw, sh, image_scale, mode)
    src = rgba if has_alpha else np.concatenate([rgba[..., :3], np.full_like(rgba[..., :1], 255)], axis=-1)
    if dw == sw:
        return src.copy()                                  # Qt returns the image itself: not premultiplied
    if mode == SMOOTH:
        return smooth_scale(premultiply(src) if has_alpha else src, dw, dh)
    return fast_scale(src, dw, dh, has_alpha)


def white_mask(rgba):
    """TwoViewStereo's mask test: 1 where r = g = b = a = 255."""
    return (rgba == 255).all(axis=-1).astype(np.uint8)


def ingest(rgba, has_alpha, image_scale, mask_rule=MASK_NONE, mask_rgba=None, mask_has_alpha=False):
    """What srh_view_upload_scaled leaves in a slot: (scaled rgba, mask bytes with 1 = WHITE)."""
    img = scale_image(rgba, has_alpha, image_scale, SMOOTH)
    h, w = img.shape[:2]
    mask = np.ones((h, w), dtype=np.uint8)
    if mask_rule == MASK_ALPHA_FAST and has_alpha:
        # MultiViewStereo: the alpha of a second, fast-scaled copy; pixels beyond that copy are not WHITE
        m = scale_image(rgba, True, image_scale, FAST)
        mh, mw = m.shape[:2]
        assert mw == w and mh <= h
        mask[:] = 0
        mask[:mh, :mw] = m[..., 3] == 255
    elif mask_rule == MASK_IMAGE_SMOOTH and mask_rgba is not None:
        # TwoViewStereo: a mask image smooth-scaled by its own width; pixels beyond it are not WHITE
        m = white_mask(scale_image(mask_rgba, mask_has_alpha, image_scale, SMOOTH))
        mh, mw = min(m.shape[0], h), min(m.shape[1], w)
        mask[:] = 0
        mask[:mh, :mw] = m[:mh, :mw]
    return img, mask


def synthetic_source(w, h, seed):
    """The synthetic sources of tests/golden/qt_scale.npz, regenerated from their seeds: uniform bytes, alpha 255 on
    about 75 % of the pixels and uniform elsewhere (the fixture keeps a checksum of each)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 3][rng.random((h, w)) < 0.75] = 255
    return img
