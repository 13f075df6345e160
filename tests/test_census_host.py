"""CPU checks of the support-weighted census cost (option "cost" = COST_CENSUS): the restatement
(tests/census_restatement.cpp) against a second, independent numpy statement of signature and cost, the library's exports
and constants, a sanity condition on the restatement's WTA against the NCC oracle, and a subclass of the host class that
calls the protected cost_census, compiled without a device."""
import math
import os
import subprocess

import numpy as np
import pytest

import cases
import census_ref as CR
import oracle_ffi as O
from stereoreconstruction_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "stereoreconstruction_amd", "host")
LIBDIR = os.path.join(ROOT, "stereoreconstruction_amd")


def _gray_plane(rgba):
    """RGBA::toGray of every pixel, in sro_to_gray's order of operations (IEEE double)"""
    r, g, b = (rgba[..., k].astype(np.float64) for k in range(3))
    return 0.11 * r + 0.59 * g + 0.3 * b


def _np_census(rgba):
    """the signature plane by whole-plane shifts: bit (dy + 3)*9 + (dx + 4) where the shifted plane is darker"""
    g = _gray_plane(rgba)
    h, w = g.shape
    sig = np.zeros((h, w), np.uint64)
    pad = np.full((h + 6, w + 8), np.inf)                     # outside the image: never darker
    pad[3:3 + h, 4:4 + w] = g
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dx == 0 and dy == 0:
                continue
            nb = pad[3 + dy:3 + dy + h, 4 + dx:4 + dx + w]
            sig |= (nb < g).astype(np.uint64) << np.uint64((dy + 3) * 9 + (dx + 4))
    return sig


def _np_cost_census(lrgba, lmask, rrgba, rmask, wts, op, x1, y1, x2, y2):
    """the census cost in plain Python floats (IEEE double; math.fma where Python has it, else exact rationals)"""
    from fractions import Fraction
    fma = getattr(math, "fma", None) or (lambda a, b, c: float(Fraction(a) * Fraction(b) + Fraction(c)))
    sl, sr = _np_census(lrgba), _np_census(rrgba)
    R = op.window_radius
    h, w = lrgba.shape[:2]
    s, tw, n = 0.0, 0.0, 0
    for row in range(-R, R + 1):
        for col in range(-R, R + 1):
            xl, yl, xr, yr = x1 + col, y1 + row, x2 + col, y2 + row
            if not (0 <= xl and 0 <= yl and xl + 1 < w and yl + 1 < h and lmask[yl, xl] == 1):
                continue
            if not (0 <= xr < w and 0 <= yr < h and rmask[yr, xr] == 1):
                continue
            wt = float(wts[row + R, col + R])
            if wt > op.weight_cutoff:
                hd = bin(int(sl[yl, xl]) ^ int(sr[yr, xr])).count("1")
                s = fma(wt, float(hd), s)
                tw += wt
                n += 1
    if n <= 4 or tw <= 1e-10:
        return op.bad_ret
    return s / tw


def _images(w=9, h=7, seed=3):
    rng = np.random.default_rng(seed)
    l = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    r = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    return l, r, np.ones((h, w), np.uint8), np.ones((h, w), np.uint8)


def _both(l, lm, r, rm, wts, op, x1, y1, x2, y2):
    got = CR.cost_census(O.OImage(l, lm), O.OImage(r, rm), wts, op, x1, y1, x2, y2)
    want = _np_cost_census(l, lm, r, rm, wts, op, x1, y1, x2, y2)
    assert CR.same_bits(np.float64(got), np.float64(want)), (got, want)
    return got


def test_signature_known_answer_9x7():
    """a 9x7 image whose gray rises along the rows and columns: the centre pixel sees every neighbour of the rows above and
    of its own row to the left as darker -- bits 0..30 -- and nothing else; a corner sees only what lies inside"""
    w, h = 9, 7
    img = np.zeros((h, w, 4), np.uint8)
    v = (np.arange(h)[:, None] * w + np.arange(w)[None, :]) * 4          # strictly rising in row-major order
    img[..., 0] = img[..., 1] = img[..., 2] = v.astype(np.uint8)
    img[..., 3] = 255
    sig = CR.census_plane(O.OImage(img, np.ones((h, w), np.uint8)))
    assert int(sig[3, 4]) == (1 << 31) - 1                                 # the 31 pixels before the centre, row-major
    assert int(sig[0, 0]) == 0                                             # the darkest pixel
    # the last pixel: everything inside its 9x7 neighbourhood is darker: dy in -3..0, dx in -4..0 without itself
    want = 0
    for dy in range(-3, 1):
        for dx in range(-4, 1):
            if (dx, dy) != (0, 0):
                want |= 1 << ((dy + 3) * 9 + (dx + 4))
    assert int(sig[h - 1, w - 1]) == want
    assert not (sig & np.uint64(1 << 31)).any() and not (sig & np.uint64(1 << 63)).any()
    assert np.array_equal(sig, _np_census(img))


@pytest.mark.parametrize("w,h", [(1, 1), (9, 1), (1, 7), (5, 5), (8, 6), (9, 7), (10, 8), (24, 19)])
def test_signature_planes_match_numpy(w, h):
    """images narrower than 9 and shorter than 7 included; equal gray values set no bit"""
    l, r, lm, rm = _images(w, h, seed=w * 31 + h)
    l[h // 2:, :, :3] = l[h // 2, 0, :3]                                   # a flat half: ties
    for img in (l, r):
        sig = CR.census_plane(O.OImage(img, lm))
        assert np.array_equal(sig, _np_census(img))
        assert not (sig & np.uint64((1 << 31) | (1 << 63))).any()
    # the mask is not consulted
    hole = lm.copy()
    hole[::2, ::2] = 0
    assert np.array_equal(CR.census_plane(O.OImage(r, hole)), CR.census_plane(O.OImage(r, rm)))


def test_cost_known_answer():
    """uniform weights, every tap counting: the cost is the mean Hamming distance of the tap pairs"""
    w, h = 12, 10
    l, r, lm, rm = _images(w, h, seed=5)
    op = O.params_twoview(window_radius=1)
    sl, sr = _np_census(l), _np_census(r)
    x1, y1, x2, y2 = 4, 4, 6, 5
    hd = [bin(int(sl[y1 + dy, x1 + dx]) ^ int(sr[y2 + dy, x2 + dx])).count("1") for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    got = _both(l, lm, r, rm, np.ones((3, 3)), op, x1, y1, x2, y2)
    assert got == sum(hd) / 9.0 and 0.0 <= got <= 62.0
    # identical images, identical position: zero
    assert _both(l, lm, l, lm, np.ones((3, 3)), op, x1, y1, x1, y1) == 0.0


def test_four_pixels_is_bad_ret_five_is_not():
    l, r, lm, rm = _images(12, 10)
    op = O.params_twoview(window_radius=1)
    wts = np.ones((3, 3))
    x1, y1 = 3, 3
    lm[:] = 0
    lm[y1, x1 - 1:x1 + 2] = 1
    lm[y1 - 1, x1] = 1                                       # numPixels == 4
    assert _both(l, lm, r, rm, wts, op, x1, y1, 4, 3) == op.bad_ret
    lm[y1 + 1, x1] = 1                                       # 5
    assert _both(l, lm, r, rm, wts, op, x1, y1, 4, 3) != op.bad_ret


def test_total_weight_at_most_1e10_is_bad_ret():
    l, r, lm, rm = _images(12, 10)
    op = O.params_twoview(window_radius=1, weight_cutoff=1e-13)
    assert _both(l, lm, r, rm, np.full((3, 3), 1e-11), op, 3, 3, 4, 3) == op.bad_ret
    assert _both(l, lm, r, rm, np.full((3, 3), 2e-11), op, 3, 3, 4, 3) != op.bad_ret


def test_last_column_and_row_count_on_the_right_not_on_the_left():
    w, h = 12, 10
    l, r, lm, rm = _images(w, h)
    op = O.params_twoview(window_radius=1)
    wts = np.arange(1.0, 10.0).reshape(3, 3)
    got = _both(l, lm, r, rm, wts, op, 3, 3, w - 2, 3)
    rm2 = rm.copy()
    rm2[:, w - 1] = 0
    assert not CR.same_bits(np.float64(got), np.float64(_both(l, lm, r, rm2, wts, op, 3, 3, w - 2, 3)))
    a = _both(l, lm, r, rm, wts, op, w - 2, 3, 3, 3)
    lm2 = lm.copy()
    lm2[:, w - 1] = 0
    assert CR.same_bits(np.float64(a), np.float64(_both(l, lm2, r, rm, wts, op, w - 2, 3, 3, 3)))
    b = _both(l, lm, r, rm, wts, op, 3, h - 2, 3, h - 2)
    lm3 = lm.copy()
    lm3[h - 1, :] = 0
    assert CR.same_bits(np.float64(b), np.float64(_both(l, lm3, r, rm, wts, op, 3, h - 2, 3, h - 2)))
    # max_color_diff is not read
    op2 = O.params_twoview(window_radius=1, max_color_diff=1.0)
    assert CR.same_bits(np.float64(got), np.float64(_both(l, lm, r, rm, wts, op2, 3, 3, w - 2, 3)))


def test_random_windows_match_numpy():
    """masks with holes, zero and sub-cut-off weights, candidates outside the image, every radius"""
    rng = np.random.default_rng(11)
    for R in (1, 2, 5):
        w, h = 24, 19
        l, r, lm, rm = _images(w, h, seed=R)
        lm[rng.random((h, w)) < 0.15] = 0
        rm[rng.random((h, w)) < 0.15] = 0
        op = O.params_twoview(window_radius=R)
        for _ in range(40):
            wts = rng.random((2 * R + 1, 2 * R + 1))
            wts[rng.random(wts.shape) < 0.1] = 0.0
            x1, y1 = int(rng.integers(0, w)), int(rng.integers(0, h))
            x2, y2 = int(rng.integers(-2, w + 2)), int(rng.integers(-2, h + 2))
            _both(l, lm, r, rm, wts, op, x1, y1, x2, y2)


def test_pair_costs_use_the_pixels_own_window():
    case = cases.get_twoview("geodesic_masks")
    imgs, ocams, op = cases.oracle_inputs(case)
    (lr, lm), (rr, rm) = case["views"][0][:2], case["views"][1][:2]
    xy = np.array([[20, 17, 12, 17], [5, 5, 9, 5], [63, 39, 63, 39], [0, 0, -2, 1], [30, 13, 22, 13]], np.int32)
    got = CR.pair_costs_census(imgs[0], imgs[1], op, xy)
    for k, (x1, y1, x2, y2) in enumerate(xy):
        want = _np_cost_census(lr, lm, rr, rm, O.weights(imgs[0], int(x1), int(y1), op), op, int(x1), int(y1), int(x2), int(y2))
        assert CR.same_bits(np.float64(got[k]), np.float64(want)), (k, got[k], want)


def _share_within_one(depth, case):
    """left-pass pixels whose winner survives the ratio test and lies within 1 px of the synthetic truth (f = w, B = 1)"""
    w = depth.shape[1]
    fin = np.isfinite(depth)
    d = np.where(fin, w / np.where(fin, depth, 1.0), np.inf)
    return int((fin & (np.abs(d - case["gt_disparity"]) <= 1.0 + 1e-6)).sum())


@pytest.mark.parametrize("name", ["geodesic_rect", "geodesic_r2"])
def test_restated_wta_is_in_the_ncc_oracles_class(name):
    """a sanity condition on the restatement alone (a broken bit order or tap rule falls far below): its count of left-pass
    pixels within 1 px of gt_disparity is at least 0.8 of the NCC oracle's on the same case"""
    case = cases.get_twoview(name)
    imgs, ocams, op = cases.oracle_inputs(case)
    census = _share_within_one(CR.twoview_wta_census(imgs[0], imgs[1], ocams[0], ocams[1], op), case)
    ncc = _share_within_one(O.twoview_wta(imgs[0], imgs[1], ocams[0], ocams[1], op), case)
    print("%s: census %d, ncc %d, ratio %.3f" % (name, census, ncc, census / ncc))
    assert ncc > 100 and census >= 0.8 * ncc


def test_library_exports_and_constants():
    L = capi.lib()
    assert hasattr(L, "srh_view_census") and "srh_view_census" in capi.EXPORTS
    assert capi.COST_CENSUS == 3 and hasattr(capi.Context, "view_census")
    hdr = open(os.path.join(ROOT, "include", "stereo_recon_hip.h")).read()
    assert "SRH_COST_CENSUS = 3" in hdr and "srh_view_census" in hdr


def test_host_subclass_calling_cost_census_compiles_without_gpu(tmp_path):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "host_census_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + HOST,
                           os.path.join(ROOT, "tests", "host_census_test.cpp"),
                           os.path.join(HOST, "libstereo_recon_host.a"),
                           "-L" + LIBDIR, "-lstereo_recon_hip", "-Wl,-rpath," + LIBDIR, "-o", exe])
    assert os.path.exists(exe)
